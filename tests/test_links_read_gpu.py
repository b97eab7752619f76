"""The native link-table reader on the device (include/ldweaver_amd.h 13) against the pure-Python yardstick tests/links_ref.py
(float() per token): exact values on three corpora, chunk boundaries, refusals with their line and column, the row-order figures, and the consumers
(LD map, Tukey + ARACNE) run from files on an engine that holds no alignment."""
import ctypes as C
import gzip
import os
import warnings

import numpy as np
import pandas as pd
import pytest

import ldw_oracle as orc
import links_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import engine as E
from ldweaver_amd import links_io as IO
from ldweaver_amd import lr as LR
from ldweaver_amd import mi as MIH
from ldweaver_amd import plots as P
from ldweaver_amd.snpdat import CdsVar, SnpDat
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu


def _native(eng, path, ncols, sep, chunk=0):
    rows, slow, ints = eng.tsv_read(path, sep, ncols, chunk)
    return [eng.tsv_fetch(k, rows) for k in range(ncols)], list(ints), slow


def _check(eng, path, ncols, sep, chunk=0):
    """Native == links_ref bit for bit, the plain-integer bits included.  Returns (rows, slow cells)."""
    cols, ints, slow = _native(eng, path, ncols, sep, chunk)
    ref, plain = R.read(path, ncols, sep)
    for k in range(ncols):
        assert R.same_bits(cols[k], ref[k]), (str(path), k, chunk)
    assert ints == plain, (ints, plain)
    return len(ref[0]), slow


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------------

def test_exact_on_the_writers_format_without_slow_cells(engine, tmp_path):
    """(a) what ldw_format_number prints of doubles with |x| in [1e-8, 1e15), and integers: at most 15 significant digits (10^15 < 2^53) and at most 22
    digits behind the point, so every cell is on the device's fast path — slow_cells must be 0, or the fast path never ran."""
    rng = np.random.default_rng(11)
    n = 200_000
    mag = lambda: np.exp(rng.uniform(np.log(1e-8), np.log(0.99e15), n)) * rng.choice([-1.0, 1.0], n)
    cols = [rng.integers(1, 9, n).astype(np.int32), rng.integers(-10**9, 10**9, n).astype(np.int64), mag(), mag(), rng.random(n) + 1e-8,
            (rng.integers(1, 3000, n) * 1000).astype(np.float64)]
    path = tmp_path / "a.tsv"
    E.write_table_tsv(str(path), cols, append=False)
    rows, slow = _check(engine, path, 6, "\t")
    assert rows == n and slow == 0
    got, ints, _ = _native(engine, path, 6, "\t")
    assert ints == [True, True, False, False, False, False]          # (1e+05 among the round thousands)
    assert np.array_equal(got[1], cols[1].astype(np.float64))


def test_exact_on_the_adversarial_corpus_with_slow_cells(engine, tmp_path):
    """(b) 16-25 digit mantissas, exponents to +-320, subnormals, halfway cases, -0, 1e+05, 1E5, .5, 5., long zero runs, every special token."""
    rng = np.random.default_rng(12)
    toks = R.adversarial_tokens(rng, 400_000)
    path = tmp_path / "b.txt"
    rows = R.write_table(path, toks, 2, sep=" ")
    assert rows >= 200_000
    got_rows, slow = _check(engine, path, 2, " ")
    assert got_rows == rows and slow > 0


def test_exact_on_reference_written_shapes(engine, tmp_path):
    """(c) positions written as doubles (1e+05), SpydrPick files of 4 and 5 space-separated columns; the frames equal pandas' round-trip read."""
    rng = np.random.default_rng(13)
    n = 200_000
    p1, p2 = (rng.integers(1, 40, n) * 50000).astype(np.float64), (rng.integers(1, 4_000_000, n)).astype(np.float64)
    ln, mi = np.abs(p1 - p2), rng.random(n) * 0.9 + 0.01
    lr = tmp_path / "lr.tsv"
    E.write_table_tsv(str(lr), [p1, p2, rng.integers(1, 4, n).astype(np.float64), rng.integers(1, 4, n).astype(np.float64), ln, mi], append=False)
    assert b"1e+05" in lr.read_bytes()[:200000]
    assert _check(engine, lr, 6, "\t") == (n, 0)
    sp4, sp5 = tmp_path / "sp4.txt", tmp_path / "sp5.txt"
    sp4.write_text("".join(f"{int(a)} {int(b)} {int(c)} {d:.6f}\n" for a, b, c, d in zip(p1, p2, ln, mi)))
    sp5.write_text("".join(f"{int(a)} {int(b)} {int(c)} {int(f)} {float(d)!r}\n" for a, b, c, d, f in zip(p1, p2, ln, mi, rng.integers(0, 2, n))))
    assert _check(engine, sp4, 4, " ")[0] == n and _check(engine, sp5, 5, " ")[0] == n
    for path, kw, kind in ((lr, dict(sep="\t", names=IO.LR_COLS), "lr"), (sp4, dict(sep=" ", names=IO.SPYDRPICK_COLS[4]), "spydrpick"),
                           (sp5, dict(sep=" ", names=IO.SPYDRPICK_COLS[5]), "spydrpick")):
        want = pd.read_csv(path, header=None, quoting=3, comment=None, float_precision="round_trip", **kw)
        want = want[~(want["len"] < 20000)].reset_index(drop=True)
        got = IO.read_links_native(path, kind, engine=engine)
        assert list(got.columns) == list(want.columns) and [str(t) for t in got.dtypes] == [str(t) for t in want.dtypes]
        for c in want.columns:
            assert R.same_bits(got[c].to_numpy(dtype=np.float64), want[c].to_numpy(dtype=np.float64)), (kind, c)
    assert P.read_LongRangeLinks(sp5, links_from_spydrpick=True, reader="native").equals(IO.read_links_native(sp5, "spydrpick", engine=engine))
    dev = IO.read_links_native(lr, "lr", engine=engine, to="device")
    assert set(dev) == set(IO.LR_COLS) and dev["MI"].is_cuda and R.same_bits(dev["MI"].cpu().numpy(), want_mi(lr))


def want_mi(path):
    cols, _ = R.read(path, 6, "\t")
    return cols[5][~(cols[4] < 20000)]


# ---- chunking -------------------------------------------------------------------------------------------------------------------------------------

def _odd_table(rng, newline):
    rows = []
    for i in range(400):
        w = int(rng.integers(1, 30))
        rows.append("\t".join([str(i), "%.*e" % (w, rng.random() * 10.0 ** int(rng.integers(-30, 30))), "0." + "0" * int(rng.integers(0, 200)) + "5"]))
    rows[100] = "100\t1" + "0" * 5000 + "\t7"              # a line longer than the small chunks
    rows.insert(50, "")
    rows.insert(200, "")
    return (newline.join(rows)).encode()                      # no final newline


@pytest.mark.parametrize("newline", ["\n", "\r\n"])
def test_chunk_sizes_give_identical_results(engine, tmp_path, newline):
    data = _odd_table(np.random.default_rng(21), newline)
    plain, gz = tmp_path / "t.tsv", tmp_path / "t.tsv.gz"
    plain.write_bytes(data)
    gz.write_bytes(gzip.compress(data))
    ref, flags = R.parse(data, 3, b"\t")
    assert len(ref[0]) == 400
    for path in (plain, gz):
        for chunk in (64, 4096, 65537, 0):
            cols, ints, slow = _native(engine, path, 3, "\t", chunk)
            assert all(R.same_bits(cols[k], ref[k]) for k in range(3)) and ints == flags and slow > 0, (str(path), chunk)
    with_nl = tmp_path / "nl.tsv"
    with_nl.write_bytes(data + newline.encode())
    assert all(R.same_bits(a, b) for a, b in zip(_native(engine, with_nl, 3, "\t", 64)[0], ref))


def test_a_carriage_return_on_either_side_of_a_chunk_boundary(engine, tmp_path):
    for pad in range(56, 70):      # the "\r\n" of the first line walks across the 64-byte boundary
        data = ("1" * pad + "\t2\r\n3\t4\r\n\r\n5\t6").encode()
        p = tmp_path / f"cr{pad}.tsv"
        p.write_bytes(data)
        cols, _, _ = _native(engine, p, 2, "\t", 64)
        ref, _ = R.parse(data, 2, b"\t")
        assert all(R.same_bits(a, b) for a, b in zip(cols, ref)) and len(cols[0]) == 3, pad


def test_empty_files(engine, tmp_path):
    for name, data in (("e0", b""), ("e1", b"\n\r\n\n")):
        p = tmp_path / name
        p.write_bytes(data)
        assert engine.tsv_read(p, "\t", 3) == (0, 0, (False, False, False))
        assert [len(c) for c in engine.tsv_columns()] == [0, 0, 0]
        df = IO.read_links_native(p, "lr", engine=engine)
        assert list(df.columns) == IO.LR_COLS and len(df) == 0


@pytest.mark.parametrize("chunk", [4096, 0])
def test_a_line_over_one_mebibyte_is_refused(engine, tmp_path, chunk):
    p = tmp_path / "long.tsv"
    p.write_bytes(b"1\t2\n3\t" + b"4" * ((1 << 20) + 8) + b"\n5\t6\n")
    with pytest.raises(L.LdwError) as e:
        engine.tsv_read(p, "\t", 2, chunk)
    assert e.value.code == L.LDW_ERR_ARG and "line 2, column 1" in str(e.value) and "longer than" in str(e.value) and "long.tsv" in str(e.value)
    ok = tmp_path / "fits.tsv"
    ok.write_bytes(b"1\t2\n3\t" + b"4" * ((1 << 20) - 16) + b"\n5\t6\n")
    assert engine.tsv_read(ok, "\t", 2, chunk)[0] == 3


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------

BAD_TABLES = {"ragged_short": "1\t2\t3\n4\t5\n", "ragged_long": "1\t2\t3\n\n4\t5\t6\t7\n", "empty_field": "1\t\t3\n", "two_points": "1\t1.2.3\t3\n",
              "hex": "1\t2\t0x10\n", "quoted": '1\t"2"\t3\n', "plus_inf": "1\t+Inf\t3\n", "bare_exponent": "1\t2e\t3\n",
              "earliest_of_two": "1\t2\t3\n" * 40 + "1\tx\t3\n" + "1\t2\t3\n" * 500 + "1\t2\n"}


@pytest.mark.parametrize("name", sorted(BAD_TABLES))
@pytest.mark.parametrize("chunk", [64, 0])
def test_refusals_name_the_line_and_the_column(engine, tmp_path, name, chunk):
    p = tmp_path / f"{name}.tsv"
    p.write_text(BAD_TABLES[name])
    with pytest.raises(R.Refused) as want:
        R.read(p, 3, "\t")
    with pytest.raises(L.LdwError) as e:
        engine.tsv_read(p, "\t", 3, chunk)
    assert e.value.code == L.LDW_ERR_ARG and f"{name}.tsv: line {want.value.line}, column {want.value.col}:" in str(e.value), (str(e.value), str(want.value))
    assert [len(c) for c in engine.tsv_columns()] == [0, 0, 0]        # no table is left behind ...
    good = tmp_path / "good.tsv"                  # ... and the context works on
    good.write_text("1\t2\t3\n")
    assert engine.tsv_read(good, "\t", 3, chunk)[0] == 1 and engine.tsv_fetch(2, 1).tolist() == [3.0]


def test_links_load_refusals(engine, tmp_path):
    engine.set_positions(np.array([100, 200, 300, 400], dtype=np.int32), 1000.0)
    cases = {"range": ("100\t200\t1\t1\t50000\t0.5\n2147483648\t200\t1\t1\t50000\t0.5\n", "line 2, column 1", "32 bits"),
             "fraction": ("100\t200\t1\t1\t50000\t0.5\n\n100\t200.5\t1\t1\t50000\t0.5\n", "line 3, column 2", "not an integer"),
             "unknown": ("100\t250\t1\t1\t50000\t0.5\n", "line 1, column 2", "no SNP's"),
             "nan": ("NA\t200\t1\t1\t50000\t0.5\n", "line 1, column 1", "not an integer")}
    for name, (text, where, why) in cases.items():
        p = tmp_path / f"{name}.tsv"
        p.write_text(text)
        assert engine.tsv_read(p, "\t", 6)[0] >= 1
        with pytest.raises(L.LdwError) as e:
            engine.links_load(1, 0, 1, 5, 4, 20000.0)
        assert e.value.code == L.LDW_ERR_ARG and where in str(e.value) and why in str(e.value) and f"{name}.tsv" in str(e.value), str(e.value)
    # a bad position in a row the len filter drops is nobody's business; the good rows load, pos1 on the to side
    p = tmp_path / "ok.tsv"
    p.write_text("300\t100\t1\t1\t50000\t0.25\n100\t250\t1\t1\t10\t0.5\n400\t200\t1\t1\tNA\t0.75\n")
    engine.tsv_read(p, "\t", 6)
    assert engine.links_load(1, 0, 1, 5, 4, 20000.0) == 2
    a, b, mi = engine.links(1)
    assert a.tolist() == [0, 1] and b.tolist() == [2, 3] and mi.tolist() == [0.25, 0.75]
    with pytest.raises(L.LdwError) as e:
        engine.links_load(1, 0, 1, 6)
    assert e.value.code == L.LDW_ERR_ARG and "column index" in str(e.value)
    # positions in another order, a position held twice: the first SNP of the position
    engine.set_positions(np.array([300, 100, 300, 200], dtype=np.int32), 1000.0)
    p2 = tmp_path / "perm.tsv"
    p2.write_text("300\t100\t1\t1\t50000\t0.25\n200\t300\t1\t1\t50000\t0.5\n")
    engine.tsv_read(p2, "\t", 6)
    assert engine.links_load(0, 0, 1, 5) == 2
    a, b, _ = engine.links(0)
    assert a.tolist() == [1, 0] and b.tolist() == [0, 3]


# ---- positions in any order: the ascending order ldw_links_load searches, shared with the position-based consumers ----------------------------------------

POS_ANY = np.array([40, 10, 30, 10, 70, 50, 20], dtype=np.int32)        # unsorted, one position held twice
POS_TIED = np.array([10, 10, 20, 30, 40, 50, 70], dtype=np.int32)       # ascending but not strictly: the path without an order array
POS_OTHER = np.array([20, 70, 10, 50, 10, 30, 40], dtype=np.int32)      # the same positions, another permutation
ANY_P1, ANY_P2, ANY_MI = [10, 70, 20, 40], [70, 20, 40, 10], [0.125, 0.25, 0.5, 0.75]


def _first_snp(POS, q):
    """The first SNP (lowest index) at every position of q, from plain numpy."""
    order = np.argsort(POS, kind="stable")
    at = np.searchsorted(POS[order], q, side="left")
    assert (POS[order][at] == q).all()
    return order[at]


def _any_table(path, extra=""):
    path.write_text("".join(f"{p1}\t{p2}\t{mi}\n" for p1, p2, mi in zip(ANY_P1, ANY_P2, ANY_MI)) + extra)
    return path


def _load_any(eng, path):
    assert eng.tsv_read(path, "\t", 3)[0] == 4
    assert eng.links_load(1, 0, 1, 2) == 4
    return eng.links(1)


@pytest.mark.parametrize("POS", [POS_ANY, POS_TIED], ids=["unsorted", "ascending_with_a_tie"])
def test_links_load_with_positions_in_any_order(tmp_path, POS):
    with E.Engine(0) as eng:
        eng.set_positions(POS, 1000.0)
        a, b, mi = _load_any(eng, _any_table(tmp_path / "any.tsv"))
        # pos2 is the from side (a), pos1 the to side (b); a position held twice is its first SNP
        assert a.tolist() == _first_snp(POS, ANY_P2).tolist() and b.tolist() == _first_snp(POS, ANY_P1).tolist() and mi.tolist() == ANY_MI
        assert b[0] == (1 if POS is POS_ANY else 0) and POS[b[0]] == 10
        bad = _any_table(tmp_path / "bad.tsv", "15\t10\t0.5\n")
        assert eng.tsv_read(bad, "\t", 3)[0] == 5
        with pytest.raises(L.LdwError) as e:
            eng.links_load(1, 0, 1, 2)
        assert e.value.code == L.LDW_ERR_ARG and "line 5, column 1: the position 15 is no SNP's" in str(e.value), str(e.value)


def test_the_position_order_survives_reuse_and_follows_new_positions(tmp_path):
    path = _any_table(tmp_path / "any.tsv")
    with E.Engine(0) as eng:
        eng.set_positions(POS_ANY, 1000.0)
        first = _load_any(eng, path)
        assert eng.ldmap(2)[1] == len(np.unique(np.r_[ANY_P1, ANY_P2]))      # (through ldw::pos_slots: four distinct positions hold links)
        again = _load_any(eng, path)
        for x, y in zip(first, again):
            assert np.array_equal(x, y)
        assert first[0].tolist() == _first_snp(POS_ANY, ANY_P2).tolist() and first[1].tolist() == _first_snp(POS_ANY, ANY_P1).tolist()
        eng.set_positions(POS_OTHER, 1000.0)
        a, b, _ = _load_any(eng, path)
        assert a.tolist() == _first_snp(POS_OTHER, ANY_P2).tolist() and b.tolist() == _first_snp(POS_OTHER, ANY_P1).tolist()
        assert a.tolist() != first[0].tolist() and b.tolist() != first[1].tolist()
        assert eng.ldmap(2)[1] == 4


# ---- row order ------------------------------------------------------------------------------------------------------------------------------------

def test_ordered_figures_equal_the_frame_route(engine, tmp_path):
    rng = np.random.default_rng(31)
    n = 5000
    sr = tmp_path / "sr.tsv"
    E.write_table_tsv(str(sr), [rng.integers(1, 4, n).astype(np.int32), rng.integers(1, 10**6, n).astype(np.int32), rng.integers(1, 10**6, n).astype(np.int32),
                                rng.integers(1, 4, n).astype(np.float64), rng.integers(1, 4, n).astype(np.float64), rng.integers(1, 20000, n).astype(np.float64),
                                rng.random(n) * 0.3, rng.random(n) * 9 + 3, rng.integers(0, 2, n).astype(np.float64)], append=False)
    lr = tmp_path / "lr.tsv"
    E.write_table_tsv(str(lr), [rng.integers(1, 10**6, n).astype(np.int32), rng.integers(1, 10**6, n).astype(np.int32), rng.integers(1, 4, n).astype(np.float64),
                                rng.integers(1, 4, n).astype(np.float64), rng.integers(10000, 10**6, n).astype(np.float64), rng.random(n) * 0.3], append=False)
    for ordered in (True, False):
        a = P.make_gwes_plots(lr_links=str(lr), sr_links=str(sr), plt_folder=str(tmp_path / f"N{ordered}"), are_srlinks_ordered=ordered, engine=engine,
                              reader="native")
        lr_ref = R.frame(lr, P.LR_COLS, "\t")
        lr_ref = lr_ref[~(lr_ref["len"] < 20000)].reset_index(drop=True)
        b = P.make_gwes_plots(lr_links=lr_ref, sr_links=R.frame(sr, P.SR_COLS, "\t"), plt_folder=str(tmp_path / f"F{ordered}"), are_srlinks_ordered=ordered,
                              engine=engine)
        assert sorted(a) == sorted(b) == ["lr_gwes", "sr_gwes_clust", "sr_gwes_combi"]
        for k in a:
            assert open(a[k], "rb").read() == open(b[k], "rb").read(), (k, ordered)
    own = P.make_gwes_plots(sr_links=str(sr), plt_folder=str(tmp_path / "own"), reader="native")          # an engine of its own
    assert open(own["sr_gwes_combi"], "rb").read() == open(a["sr_gwes_combi"], "rb").read()
    with pytest.raises(ValueError, match="^lr_links must either be"):
        P.make_gwes_plots(lr_links=str(sr), plt_folder=str(tmp_path / "x"), engine=engine, reader="native")


# ---- the consumers, from files, on an engine without an alignment -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def job(sample, tmp_path_factory):
    """perform_MI_computation on the reference's bundled sample: both tsv files, and their parsed values by the yardstick."""
    d = tmp_path_factory.mktemp("job")
    sd = SnpDat(states=sample["states"], POS=sample["POS"], g=sample["g"], uqe=sample["uqe"], r=sample["r"])
    with E.Engine(0) as eng:
        MIH.perform_MI_computation(sd, sample["hdw"], CdsVar(paint=sample["paint"], nclust=3), lr_save_path=str(d / "lr_links.tsv"),
                                   sr_save_path=str(d / "sr_links.tsv"), plt_folder=str(d / "PLOTS"), engine=eng, verbose=False)
    lr = R.frame(d / "lr_links.tsv", IO.LR_COLS, "\t")
    lr = lr[~(lr["len"] < 20000)].reset_index(drop=True)
    sr = R.frame(d / "sr_links.tsv", IO.SR_COLS, "\t")
    POS = np.unique(np.concatenate([lr["pos1"], lr["pos2"], sr["pos1"], sr["pos2"]])).astype(np.int64)
    idx = lambda p: np.searchsorted(POS, p.to_numpy()).astype(np.int32)
    tabs = dict(lr=(idx(lr["pos2"]), idx(lr["pos1"]), lr["MI"].to_numpy(dtype=np.float64)), sr=(idx(sr["pos2"]), idx(sr["pos1"]), sr["MI"].to_numpy(dtype=np.float64)))
    assert len(lr) > 1000 and len(sr) > 100
    return dict(dir=d, lr=lr, sr=sr, POS=POS, tabs=tabs, g=sample["g"])


def _import_route(job):
    """An engine that is handed the parsed values the way it always was: an alignment of that many SNPs, the meta data, links_import."""
    POS = job["POS"]
    st = np.ascontiguousarray(synth_alignment(len(POS), 16, seed=3)["states"])
    uqe, r = orc.uqe_r(st)
    eng = E.Engine(0)
    eng.set_alignment(st)
    eng.set_snp_meta(r, uqe, POS.astype(np.int32), np.ones(len(POS), dtype=np.int32), float(job["g"]))
    eng.links_import(1, *job["tabs"]["lr"])
    eng.links_import(0, *job["tabs"]["sr"])
    return eng


def test_ldmap_from_files_without_an_alignment(job, tmp_path):
    d = job["dir"]
    with E.Engine(0) as fresh, _import_route(job) as old:
        out = LR.genomewide_LDMap(fresh, lr_links_path=d / "lr_links.tsv", sr_links_path=d / "sr_links.tsv", reducer=4)
        htm, n_pos, r = old.ldmap(4)
        assert out["n_pos"] == n_pos == len(job["POS"]) and out["reducer"] == r
        assert np.array_equal(out["htm"], htm, equal_nan=True)                     # bit for bit with the links_import route
        t = lambda f: dict(pos1=f["pos1"].to_numpy(), pos2=f["pos2"].to_numpy(), MI=f["MI"].to_numpy(dtype=np.float64))
        ref = orc.ld_map(t(job["lr"]), t(job["sr"]), reducer=4, from_=None, to=None)
        np.testing.assert_allclose(out["htm"], ref["htm"], rtol=0, atol=1e-12, equal_nan=True)
        # a SpydrPick copy of the long-range file (pos1 pos2 len MI, space separated) gives the same map
        sp = tmp_path / "sp4.txt"
        sp.write_text("".join(" ".join(ln.split("\t")[k] for k in (0, 1, 4, 5)) + "\n" for ln in (d / "lr_links.tsv").read_text().splitlines()))
        out2 = LR.genomewide_LDMap(fresh, lr_links_path=sp, sr_links_path=d / "sr_links.tsv", links_from_spydrpick=True, reducer=4, plot_save_path=tmp_path / "LD.png")
        assert np.array_equal(out2["htm"], htm, equal_nan=True) and os.path.getsize(tmp_path / "LD.png") > 1000
        # with snp_dat (positions alone are taken from it) the same again
        class SD:
            POS, g = job["POS"], job["g"]
        with E.Engine(0) as e3:
            out3 = LR.genomewide_LDMap(e3, SD, reducer=4, lr_links_path=d / "lr_links.tsv", sr_links_path=d / "sr_links.tsv")
            assert np.array_equal(out3["htm"], htm, equal_nan=True)


def test_analyse_long_range_links_from_files_without_an_alignment(job, tmp_path):
    d, (a, b, mi), (sa, sb, smi), POS = job["dir"], job["tabs"]["lr"], job["tabs"]["sr"], job["POS"]
    with E.Engine(0) as fresh, _import_route(job) as old, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = LR.analyse_long_range_links(fresh, lr_links_path=d / "lr_links.tsv", sr_links_path=d / "sr_links.tsv", lr_plt_path=tmp_path / "lr_gwes.png",
                                          are_lrlinks_ordered=True)
        info = old.lr_tukey(5000, sr=(sa, sb, smi))
        red, flags = old.lr_reduced(), old.aracne_device()
        assert np.array_equal(out["q13"], info["q13"]) and np.array_equal(out["thresholds"], info["thresholds"]) and out["fallback"] == info["fallback"]
        assert out["n_pool"] == info["n_pool"]
        df = out["lr_links_red"]
        assert np.array_equal(df["pos1"], POS[red["b"]]) and np.array_equal(df["pos2"], POS[red["a"]]) and np.array_equal(df["MI"], red["MI"])
        assert np.array_equal(df["ARACNE"], flags.astype(int))
        assert np.array_equal(df["len"], job["lr"]["len"].to_numpy()[red["row"]])             # len is the file's
        assert os.path.getsize(tmp_path / "lr_gwes.png") > 1000
        # the oracle on the same parsed input
        ref = orc.analyse_long_range_links(dict(pos1=POS[b], pos2=POS[a], MI=mi), dict(pos1=POS[sb], pos2=POS[sa], MI=smi), min_links=5000)
        assert np.array_equal(ref["thresholds"], out["thresholds"]) and ref["fallback"] == out["fallback"] and ref["n_pool"] == out["n_pool"]
        o = np.argsort(-red["MI"], kind="stable")
        assert np.array_equal(red["row"][o], ref["rows"]) and np.array_equal(flags[o], ref["ARACNE"])
        # the default order: descending MI
        out_d = LR.analyse_long_range_links(fresh, lr_links_path=d / "lr_links.tsv", sr_links_path=d / "sr_links.tsv")
        assert np.array_equal(out_d["lr_links_red"]["MI"], red["MI"][o]) and np.array_equal(out_d["lr_links_red"]["ARACNE"], flags[o].astype(int))
        # the long-range figure of the library itself needs no more than the positions and g
        fresh.set_positions(POS.astype(np.int32), float(job["g"]))
        fresh.tsv_read(d / "lr_links.tsv", "\t", 6)
        fresh.links_load(1, 0, 1, 5, 4, 20000.0)
        fresh.lr_tukey(5000, sr=(sa, sb, smi))
        assert np.array_equal(fresh.aracne_device(), flags)
        o_lr = P.plot_opts(L.PLOT_LR, layer_rgb=(P.GREY, P.LR_DIRECT), hline=float(np.max(info["thresholds"])))
        P.render_links(fresh, 1, opts=o_lr, path=tmp_path / "lib.png")
        P.render_links(old, 1, opts=o_lr, path=tmp_path / "old.png")
        assert (tmp_path / "lib.png").read_bytes() == (tmp_path / "old.png").read_bytes() == (tmp_path / "lr_gwes.png").read_bytes()


def test_a_spydrpick_file_with_flags_keeps_them(job, tmp_path, monkeypatch):
    d = job["dir"]
    lines = (d / "lr_links.tsv").read_text().splitlines()
    sp = tmp_path / "sp5.txt"
    sp.write_text("".join(" ".join([*(ln.split("\t")[k] for k in (0, 1, 4)), str(i % 2), ln.split("\t")[5]]) + "\n" for i, ln in enumerate(lines)))
    file_flags = R.frame(sp, IO.SPYDRPICK_COLS[5], " ")
    file_flags = file_flags[~(file_flags["len"] < 20000)].reset_index(drop=True)["ARACNE"].to_numpy()
    with E.Engine(0) as fresh, _import_route(job) as old, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        def never(*a, **k):
            raise AssertionError("ARACNE ran although the file brings its flags")
        monkeypatch.setattr(fresh, "aracne_device", never)
        out = LR.analyse_long_range_links(fresh, lr_links_path=sp, sr_links_path=d / "sr_links.tsv", links_from_spydrpick=True, are_lrlinks_ordered=True)
        old.lr_tukey(5000, sr=job["tabs"]["sr"])
        rows = old.lr_reduced()["row"]
        assert np.array_equal(out["lr_links_red"]["ARACNE"], file_flags[rows]) and "clust1" not in out["lr_links_red"].columns


# ---- state ----------------------------------------------------------------------------------------------------------------------------------------

def test_a_position_only_context_refuses_what_needs_more(tmp_path):
    lib = L.lib()
    with E.Engine(0) as eng:
        eng.set_positions(np.arange(1, 101, dtype=np.int32) * 10, 5000.0)
        msg = lambda: lib.ldw_last_error().decode()
        w = np.ones(16)
        assert lib.ldw_set_weights(eng._ctx, L.ptr(w), 16, 0) == L.LDW_ERR_STATE
        assert lib.ldw_hamming_weights(eng._ctx, 3, L.ptr(w), None) == L.LDW_ERR_STATE
        assert lib.ldw_get_alignment(eng._ctx, L.ptr(np.zeros(1600, dtype=np.uint8))) == L.LDW_ERR_STATE
        q = np.zeros(3 * 19999)
        assert lib.ldw_sr_len_quantiles(eng._ctx, 3, 20000.0, 0.95, 19999, L.ptr(q), L.ptr(q.copy()), L.ptr(np.zeros(3 * 19999, dtype=np.int64))) == L.LDW_ERR_STATE
        assert "positions only" in msg()
        n, nb = C.c_int64(0), C.c_int64(0)
        assert lib.ldw_write_links_tsv(eng._ctx, 1, os.fsencode(tmp_path / "x.tsv"), 0, 1, C.byref(n), C.byref(nb)) == L.LDW_ERR_STATE
        blocks = np.array([[1, 100, 1, 100]], dtype=np.int32)
        prm = L.MIParams(20000.0, 1e6, 1.0, 0, 0, 1, 0)
        assert lib.ldw_mi_all_pairs(eng._ctx, L.ptr(blocks), 1, C.byref(prm), 1) == L.LDW_ERR_STATE
        # g = 0: the long-range figure cannot take len from the positions
        eng.set_positions(np.arange(1, 101, dtype=np.int32) * 10, 0.0)
        eng.links_import(1, np.arange(50, dtype=np.int32), np.arange(50, 100, dtype=np.int32), np.r_[np.linspace(0.1, 0.11, 45), np.full(5, 0.9)])
        assert eng.lr_tukey(3)["n_red"] == 5
        eng.aracne_device()
        o = P.plot_opts(L.PLOT_LR, layer_rgb=(P.GREY, P.LR_DIRECT))
        assert lib.ldw_plot_links(eng._ctx, 1, 1, C.byref(o), os.fsencode(tmp_path / "p.png"), None, None) == L.LDW_ERR_STATE and "genome length" in msg()
        # an alignment brings everything back
        syn = synth_alignment(64, 16, seed=1)
        eng.set_alignment(np.ascontiguousarray(syn["states"]))
        assert len(eng.hamming_weights(6)) == 16


def test_columns_grow_and_pinned_buffers_are_released(tmp_path):
    small, big = tmp_path / "s.tsv", tmp_path / "b.tsv.gz"
    small.write_text("1\t2\n" * 10)
    big.write_bytes(gzip.compress(b"3\t4.5\n" * 300_000))
    with E.Engine(0) as eng:
        assert eng.tsv_read(small, "\t", 2)[0] == 10
        g0 = eng.tsv_stats()["grows"]
        assert eng.tsv_read(big, "\t", 2, 1 << 16)[0] == 300_000                 # a gzip file is not sized ahead: geometric growth, chunk by chunk
        st = eng.tsv_stats()
        assert st["grows"] > g0 and st["chunks"] > 10 and st["pinned_bytes"] > 0
        c = eng.tsv_columns()
        assert float(c[0].sum()) == 900_000.0 and float(c[1].sum()) == 1_350_000.0
        assert eng.host_trim() >= st["pinned_bytes"] and eng.tsv_stats()["pinned_bytes"] == 0
        assert eng.tsv_read(small, "\t", 2)[0] == 10 and eng.tsv_fetch(1, 10).tolist() == [2.0] * 10      # ... and come back on demand
    with E.Engine(0) as eng:       # both forms of the parse kernel give the same table
        L.check(L.lib().ldw_tsv_set_variant(eng._ctx, 1))
        assert eng.tsv_read(big, "\t", 2)[0] == 300_000 and float(eng.tsv_columns()[1].sum()) == 1_350_000.0


# ---- argument refusals of the entry points that need a context -----------------------------------------------------------------------------------------

def test_argument_refusals_with_their_messages(tmp_path):
    lib = L.lib()
    msg = lambda: lib.ldw_last_error().decode()
    good = tmp_path / "g.tsv"
    good.write_text("100\t200\t0.5\n300\t400\t0.25\n")
    path = os.fsencode(good)
    rows, slow, mask = C.c_int64(0), C.c_int64(0), C.c_uint32(0)
    out = (C.byref(rows), C.byref(slow), C.byref(mask))
    p, n, nc, st = C.c_void_p(0), C.c_int64(0), C.c_int32(0), C.c_int64(0)
    d = np.zeros(4)
    with E.Engine(0) as eng:
        ctx = eng._ctx
        # before the first read
        assert lib.ldw_tsv_columns(ctx, C.byref(p), C.byref(n), C.byref(nc), C.byref(st)) == L.LDW_ERR_STATE and "ldw_tsv_columns: no table has been read" in msg()
        assert lib.ldw_tsv_fetch(ctx, 0, L.ptr(d), 4, 0) == L.LDW_ERR_STATE and "ldw_tsv_fetch: no table has been read" in msg()
        assert lib.ldw_links_load(ctx, 1, 0, 1, 2, -1, 0.0, 0, None) == L.LDW_ERR_STATE and "ldw_links_load: no table has been read" in msg()
        # ldw_tsv_read
        assert lib.ldw_tsv_read(ctx, None, 9, 3, 0, *out) == L.LDW_ERR_ARG and msg() == "ldw_tsv_read: null path"
        for sep in (ord(","), 0, ord("\n")):
            assert lib.ldw_tsv_read(ctx, path, sep, 3, 0, *out) == L.LDW_ERR_ARG and f"the separator must be a tab or a space (got {sep})" in msg()
        for bad in (0, 17, -1):
            assert lib.ldw_tsv_read(ctx, path, 9, bad, 0, *out) == L.LDW_ERR_ARG and f"ldw_tsv_read: ncols = {bad} outside 1..16" in msg()
        for bad in (-1, (1 << 30) + 1):
            assert lib.ldw_tsv_read(ctx, path, 9, 3, bad, *out) == L.LDW_ERR_ARG and f"ldw_tsv_read: chunk_bytes = {bad} outside 0..2^30" in msg()
        assert lib.ldw_tsv_read(ctx, os.fsencode(tmp_path / "nothing"), 9, 3, 0, *out) == L.LDW_ERR_ARG and "cannot open" in msg()
        with pytest.raises(FileNotFoundError):
            eng.tsv_read(tmp_path / "nothing", "\t", 3)
        assert lib.ldw_tsv_read(ctx, path, 9, 3, 0, None, None, None) == L.LDW_OK          # every output may be NULL
        assert lib.ldw_tsv_read(ctx, path, 9, 3, 1 << 20, *out) == L.LDW_OK and rows.value == 2 and mask.value == 0b011
        # ldw_tsv_columns / ldw_tsv_fetch
        assert lib.ldw_tsv_columns(ctx, None, C.byref(n), C.byref(nc), C.byref(st)) == L.LDW_ERR_ARG and msg() == "ldw_tsv_columns: null argument"
        assert lib.ldw_tsv_columns(ctx, C.byref(p), C.byref(n), C.byref(nc), C.byref(st)) == L.LDW_OK and (n.value, nc.value) == (2, 3) and st.value >= 2
        for col in (-1, 3):
            assert lib.ldw_tsv_fetch(ctx, col, L.ptr(d), 4, 0) == L.LDW_ERR_ARG and f"ldw_tsv_fetch: column {col} outside 0..2" in msg()
        assert lib.ldw_tsv_fetch(ctx, 0, L.ptr(d), 1, 0) == L.LDW_ERR_SIZE and "ldw_tsv_fetch: capacity 1 < 2 rows" in msg()
        assert lib.ldw_tsv_fetch(ctx, 0, None, 4, 0) == L.LDW_ERR_ARG and msg() == "ldw_tsv_fetch: null output"
        assert lib.ldw_tsv_fetch(ctx, 2, L.ptr(d), 4, 0) == L.LDW_OK and d[:2].tolist() == [0.5, 0.25]
        # ldw_links_load without positions
        assert lib.ldw_links_load(ctx, 1, 0, 1, 2, -1, 0.0, 0, None) == L.LDW_ERR_STATE and "ldw_links_load: no positions" in msg()
        # ldw_set_positions
        pos = np.array([100, 200, 300, 400], dtype=np.int32)
        assert lib.ldw_set_positions(ctx, None, 4, 1000.0) == L.LDW_ERR_ARG and "ldw_set_positions: null positions or L = 4" in msg()
        for bad in (0, -3, 1 << 27):
            assert lib.ldw_set_positions(ctx, L.ptr(pos), bad, 1000.0) == L.LDW_ERR_ARG and f"L = {bad} outside 1..2^27" in msg()
        for bad in (-1.0, float("nan")):
            assert lib.ldw_set_positions(ctx, L.ptr(pos), 4, bad) == L.LDW_ERR_ARG and "ldw_set_positions: genome length g must be positive, or 0" in msg()
        assert lib.ldw_links_load(ctx, 1, 0, 1, 2, -1, 0.0, 0, None) == L.LDW_ERR_STATE           # (the refused calls set nothing)
        assert lib.ldw_set_positions(ctx, L.ptr(pos), 4, 1000.0) == L.LDW_OK
        # ldw_links_load
        for which in (-1, 2):
            assert lib.ldw_links_load(ctx, which, 0, 1, 2, -1, 0.0, 0, None) == L.LDW_ERR_ARG and msg() == "ldw_links_load: which must be 0 (sr) or 1 (lr)"
        assert lib.ldw_links_load(ctx, 1, 0, 1, 2, -1, 0.0, 1, None) == L.LDW_ERR_ARG and msg() == "ldw_links_load: flags must be 0"
        for cols in ((3, 1, 2, -1), (0, -1, 2, -1), (0, 1, 3, -1), (0, 1, 2, -2), (0, 1, 2, 3)):
            assert lib.ldw_links_load(ctx, 1, *cols, 0.0, 0, None) == L.LDW_ERR_ARG and "a column index lies outside the 3 columns read" in msg()
        kept = C.c_int64(-1)
        assert lib.ldw_links_load(ctx, 1, 0, 1, 2, -1, 0.0, 0, C.byref(kept)) == L.LDW_OK and kept.value == 2
        # both positions of a row are bad: the leftmost FILE column is named, whichever of pos1 / pos2 it is
        both = tmp_path / "both.tsv"
        both.write_text("100\t200\t0.5\n150\t250\t0.5\n")
        eng.tsv_read(both, "\t", 3)
        assert lib.ldw_links_load(ctx, 1, 1, 0, 2, -1, 0.0, 0, None) == L.LDW_ERR_ARG and "line 2, column 1: the position 150 is no SNP's" in msg()
        assert lib.ldw_links_load(ctx, 1, 0, 1, 2, -1, 0.0, 0, None) == L.LDW_ERR_ARG and "line 2, column 1: the position 150 is no SNP's" in msg()


def test_python_layer_limits(engine, tmp_path):
    big = tmp_path / "big.tsv"
    big.write_text("1\t100\t200\t1\t1\t100\t0.5\t4\t9007199254740993\n")
    with pytest.raises(ValueError, match="2\\^53 or beyond"):
        IO.read_links_native(big, "sr", engine=engine)
    assert IO.read_links_native(big, "sr", engine=engine, to="device")["ARACNE"].item() == 9007199254740992.0      # (the device column is the rounded double)
    # an engine that holds an alignment is never emptied behind the caller's back
    lr = tmp_path / "lr.tsv"
    lr.write_text("100\t50100\t1\t2\t50000\t0.11\n")
    syn = synth_alignment(64, 16, seed=1)
    st = np.ascontiguousarray(syn["states"])
    uqe, r = orc.uqe_r(st)

    class SD:
        POS, g = np.arange(64) * 1000 + 100, 100000.0
    with E.Engine(0) as eng:
        eng.set_alignment(st)
        with pytest.raises(ValueError, match="cannot be compared"):
            LR.genomewide_LDMap(eng, SD, reducer=2, lr_links_path=lr)
        eng.set_snp_meta(r, uqe, (SD.POS + 1).astype(np.int32), None, SD.g)
        with pytest.raises(ValueError, match="differs from the positions the engine holds"):
            LR.genomewide_LDMap(eng, SD, reducer=2, lr_links_path=lr)
        assert eng.get_alignment().shape == (64, 16)                     # still there
        eng.set_snp_meta(r, uqe, SD.POS.astype(np.int32), None, SD.g)
        assert LR.genomewide_LDMap(eng, SD, reducer=2, lr_links_path=lr)["n_pos"] == 2 and eng.get_alignment().shape == (64, 16)


# ---- the LD map's sums do not depend on the order the links arrive in ------------------------------------------------------------------------------------

def _ldmap_of(eng, POS, a, b, mi, reducer):
    eng.set_positions(POS, 0.0)
    eng.links_import(1, a, b, mi)
    return eng.ldmap(reducer)[0]


def test_ldmap_sums_are_order_independent_and_exact():
    """Cells that take many links with values of both signs and very different sizes: the map equals the one computed from the EXACT cell sums
    (Python fractions, rounded once) wherever the device's fixed point holds the values exactly, is the same on every run and for every row
    order, and values from 2^36 up, infinities and NaN still go through."""
    from fractions import Fraction
    rng = np.random.default_rng(41)
    L_, r, n = 40, 4, 60_000
    POS = (np.arange(L_, dtype=np.int32) + 1) * 100
    a, b = rng.integers(0, L_, n).astype(np.int32), rng.integers(0, L_, n).astype(np.int32)
    chain = np.arange(L_ - 1, dtype=np.int32)                       # every position occurs
    a, b = np.r_[chain, a], np.r_[chain + 1, b]
    # multiples of 2^-60 below 2^5, both signs: exact in the accumulator (units of 2^-90), sums that carry into its high word (from 2^-26 up)
    mi = np.ldexp(rng.integers(1, 1 << 52, len(a)).astype(np.float64), rng.integers(-60, -47, len(a))) * rng.choice([-1.0, 1.0], len(a))
    B = L_ // r
    exact = [[Fraction(0)] * B for _ in range(B)]
    for x, y, v in zip(a // r, b // r, mi):
        lo, hi = (x, y) if x <= y else (y, x)
        exact[lo][hi] += Fraction(float(v)) * (2 if lo == hi else 1)
    s = np.array([[float(exact[min(i, j)][max(i, j)]) for j in range(B)] for i in range(B)])
    assert (s < 0).any() and (s > 0).any() and (np.abs(s) > 2.0 ** -26).all()
    with np.errstate(invalid="ignore"):
        want = np.log10(s / (r * r) + 1e-5)                            # (a negative cell sum has no logarithm: NaN, as in R)
    want = (want - np.nanmin(want)) / (np.nanmax(want) - np.nanmin(want))
    fill = np.full(len(chain), 0.5)
    with E.Engine(0) as e1, E.Engine(0) as e2:
        h1 = _ldmap_of(e1, POS, a, b, mi, r)
        np.testing.assert_allclose(h1, want, rtol=0, atol=1e-13, equal_nan=True)
        assert np.isnan(h1).any() and np.nanmax(h1) == 1.0 and np.nanmin(h1) == 0.0
        for rep in range(3):
            assert np.array_equal(e1.ldmap(r)[0], h1, equal_nan=True)                       # run to run
        perm = rng.permutation(len(a))
        assert np.array_equal(_ldmap_of(e2, POS, a[perm], b[perm], mi[perm], r), h1, equal_nan=True)     # any row order, another context
        # past the accumulator (64 and more, infinities, NaN): one such link (1, 2) inside block 0, the chain's links of 0.5 everywhere
        one = lambda v: _ldmap_of(e2, POS, np.r_[chain, np.int32(1)], np.r_[chain + 1, np.int32(2)], np.r_[fill, v], r)
        for v in (64.0, 2.0 ** 40):
            h = one(v)
            assert h[0, 0] == 1.0 and np.isfinite(h).all() and h.min() == 0.0 and (h[1:, 1:] < 0.9).all()       # it arrived: the largest cell by far
        lone = one(63.0)                                                 # the same through the accumulator: the neighbouring value, the same picture
        assert lone[0, 0] == 1.0 and np.isfinite(lone).all() and (lone[1:, 1:] < 0.9).all()
        h = one(np.nan)
        assert np.isnan(h[0, 0]) and np.isnan(h).sum() == 1 and np.nanmax(h) == 1.0
        h = one(-2.0 ** 40)
        assert np.isnan(h[0, 0]) and np.isnan(h).sum() == 1 and np.nanmax(h) == 1.0
        h = one(np.inf)                                                  # an infinite cell makes the range infinite: (inf - min) / inf, and 0 elsewhere
        assert np.isnan(h[0, 0]) and np.isnan(h).sum() == 1 and np.nanmax(h) == 0.0


# ---- both forms of the parse kernel over the corpora that stress their bounds -------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 1])
def test_parse_kernel_forms_on_the_odd_corpora(tmp_path, variant):
    rng = np.random.default_rng(51)
    adv = tmp_path / "adv.txt"
    R.write_table(adv, R.adversarial_tokens(rng, 40_000), 3, sep=" ")
    wide = tmp_path / "wide.tsv"                 # rows of ~400 bytes: 256 of them do not fit the staged tile, the block falls back
    wide.write_text("".join("\t".join("0." + "0" * 90 + str(int(v)) for v in rng.integers(1, 10**6, 4)) + "\n" for _ in range(3000)))
    with E.Engine(0) as eng:
        L.check(L.lib().ldw_tsv_set_variant(eng._ctx, variant))
        assert _check(eng, adv, 3, " ")[1] > 0
        assert _check(eng, wide, 4, "\t")[0] == 3000
        for newline in ("\n", "\r\n"):
            data = _odd_table(np.random.default_rng(21), newline)
            p = tmp_path / f"odd{len(newline)}.tsv"
            p.write_bytes(data)
            for chunk in (64, 4096, 0):
                _check(eng, p, 3, "\t", chunk)
        assert L.lib().ldw_tsv_set_variant(eng._ctx, 2) == L.LDW_ERR_ARG
