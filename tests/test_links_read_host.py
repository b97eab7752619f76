"""The host side of the native link-table reader (include/ldweaver_amd.h 13): the pure-Python yardstick tests/links_ref.py against
pandas' round-trip parser, ldw_tsv_probe, the refusals of the new entry points that need no device, and the ``reader=`` keyword.  Runs without a GPU."""
import ctypes as C
import gzip
import os

import numpy as np
import pandas as pd
import pytest

import links_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import engine as E
from ldweaver_amd import links_io as IO
from ldweaver_amd import lr as LR
from ldweaver_amd import plots as P


def _pandas(path, sep, round_trip=True):
    return pd.read_csv(path, sep=sep, header=None, quoting=3, comment=None, **(dict(float_precision="round_trip") if round_trip else {}))


def _same_frame(ref: pd.DataFrame, pdf: pd.DataFrame):
    assert ref.shape == pdf.shape
    for k in range(ref.shape[1]):
        a, b = ref.iloc[:, k], pdf.iloc[:, k]
        assert a.dtype == b.dtype, (k, a.dtype, b.dtype)
        assert R.same_bits(a.to_numpy(dtype=np.float64), b.to_numpy(dtype=np.float64)), k
        if a.dtype == np.int64:
            assert np.array_equal(a.to_numpy(), b.to_numpy())


def _fmt(x):
    return E.format_number(x)


def test_links_ref_equals_pandas_round_trip_on_generated_corpora(tmp_path):
    rng = np.random.default_rng(2024)
    toks = R.writer_tokens(rng, 20000, _fmt)
    # (pandas keeps a column as text when a decimal token overflows to infinity, which float() and the native reader accept: such tokens are left
    # to the device test, where the yardstick is float() alone)
    adv = [t for t in R.adversarial_tokens(rng, 20000) if t.encode() in R.SPECIAL or np.isfinite(float(t))]
    n_default_differs = 0
    for name, tk, sep in (("writer", toks, "\t"), ("adversarial", adv, " ")):
        path = tmp_path / f"{name}.txt"
        R.write_table(path, tk, 4, sep=sep)
        ref = R.frame(path, [0, 1, 2, 3], sep)
        _same_frame(ref, _pandas(path, sep))
        dflt = _pandas(path, sep, round_trip=False)
        for k in range(4):
            a, b = ref.iloc[:, k].to_numpy(dtype=np.float64), dflt.iloc[:, k].to_numpy(dtype=np.float64)
            ok = (a == b) | (np.isnan(a) & np.isnan(b))
            n_default_differs += int((~ok).sum())
    # information for the later decision to flip the default reader, not an assertion
    print(f"tokens on which pandas' DEFAULT float parser differs from float(): {n_default_differs} of {len(toks) + len(adv)}")


def test_links_ref_equals_pandas_on_integer_and_mixed_columns(tmp_path):
    path = tmp_path / "m.tsv"
    path.write_text("1\t1e+05\t-0\t0.5\n+2\t200000\t7\tNA\n007\t3\t-9\tInf\n")
    ref = R.frame(path, list("abcd"), "\t")
    assert [str(t) for t in ref.dtypes] == ["int64", "float64", "int64", "float64"]
    _same_frame(ref, _pandas(path, "\t"))
    assert ref["a"].tolist() == [1, 2, 7] and ref["b"].tolist() == [100000.0, 200000.0, 3.0] and np.isnan(ref["d"][1])


def test_links_ref_equals_pandas_on_the_writers_files(tmp_path):
    rng = np.random.default_rng(5)
    n = 5000
    cols = [rng.integers(1, 4, n).astype(np.int32), rng.integers(1, 5_000_000, n).astype(np.int64), (rng.integers(50, 150, n) * 1000).astype(np.float64),
            rng.random(n), np.exp(rng.uniform(-18, 30, n))]
    path = tmp_path / "w.tsv"
    E.write_table_tsv(str(path), cols, append=False)
    ref = R.frame(path, list("abcde"), "\t")
    _same_frame(ref, _pandas(path, "\t"))
    assert [str(t) for t in ref.dtypes] == ["int64", "int64", "float64", "float64", "float64"]     # 1e+05 among the round thousands: a double column
    assert np.array_equal(ref["b"].to_numpy(), cols[1])


def test_links_ref_equals_pandas_on_the_reader_test_files(tmp_path):
    files = {"sr.tsv": ("1\t100\t2300\t1\t1\t2200\t0.31\t4.5\t1\n2\t500\t900\t2\t3\t400\t0.2\t3.25\t0\n", "\t", 9),
             "lr.tsv": ("100\t50000\t1\t2\t49900\t0.11\n200\t9000\t1\t1\t8800\t0.5\n300\t90000\t2\t2\t89700\t0.07\n", "\t", 6),
             "sp5.txt": ("100 50000 49900 1 0.11\n200 9000 8800 0 0.5\n", " ", 5),
             "sp4.txt": ("100 50000 49900 0.11\n200 90000 89800 0.5\n", " ", 4)}
    for name, (text, sep, nc) in files.items():
        p = tmp_path / name
        p.write_text(text)
        _same_frame(R.frame(p, list(range(nc)), sep), _pandas(p, sep))


@pytest.mark.parametrize("text,line,col", [("1 2 3\n1 2\n", 2, 3), ("1 2 3\n\n1 2 3 4\n", 3, 4), ("1  3\n", 1, 2), ("1 1.2.3 3\n", 1, 2), ("1 2 0x10\n", 1, 3),
                                           ('1 "2" 3\n', 1, 2), ("1 2 3\n1 x 3\n1 2\n", 2, 2), ("1 2 3\r\n\r\n1 2 3 \r\n", 3, 4), ("1 +Inf 3\n", 1, 2),
                                           ("1 1e 3\n", 1, 2), ("1 1_0 3\n", 1, 2), ("1 2 3x", 1, 3)])
def test_links_ref_refusals(text, line, col):
    with pytest.raises(R.Refused) as e:
        R.parse(text.encode(), 3, b" ")
    assert (e.value.line, e.value.col) == (line, col)


def test_links_ref_line_rules():
    cols, plain = R.parse(b"\n1\t2\r\n\r\n\n3\t4.5", 2, b"\t")
    assert cols[0].tolist() == [1.0, 3.0] and cols[1].tolist() == [2.0, 4.5] and plain == [True, False]
    cols, plain = R.parse(b"", 3, b"\t")
    assert [len(c) for c in cols] == [0, 0, 0] and plain == [False] * 3


def _probe(path, sep="\t"):
    n, gz = C.c_int32(-1), C.c_int32(-1)
    rc = L.lib().ldw_tsv_probe(os.fsencode(path), ord(sep), C.byref(n), C.byref(gz))
    return rc, n.value, gz.value


def test_tsv_probe(tmp_path):
    p = tmp_path / "a.tsv"
    p.write_text("1\t2\t3\n4\t5\t6\n")
    assert _probe(p) == (L.LDW_OK, 3, 0) and _probe(p, " ") == (L.LDW_OK, 1, 0)
    g = tmp_path / "a.tsv.gz"
    g.write_bytes(gzip.compress(b"1 2 3 4 5\n"))
    assert _probe(g, " ") == (L.LDW_OK, 5, 1)
    e = tmp_path / "empty"
    e.write_bytes(b"")
    assert _probe(e) == (L.LDW_OK, 0, 0)
    (tmp_path / "blank").write_bytes(b"\n\r\n\n")
    assert _probe(tmp_path / "blank")[:2] == (L.LDW_OK, 0)
    (tmp_path / "nonl").write_bytes(b"1\t2\t3\t4")
    assert _probe(tmp_path / "nonl")[:2] == (L.LDW_OK, 4)
    (tmp_path / "crlf").write_bytes(b"\r\n1\t2\r\n3\t4\r\n")
    assert _probe(tmp_path / "crlf")[:2] == (L.LDW_OK, 2)
    rc, _, _ = _probe(tmp_path / "no_such_file")
    assert rc == L.LDW_ERR_ARG and "cannot open" in L.lib().ldw_last_error().decode() and "no_such_file" in L.lib().ldw_last_error().decode()
    assert L.lib().ldw_tsv_probe(None, 9, None, None) == L.LDW_ERR_ARG
    n = C.c_int32(0)
    assert L.lib().ldw_tsv_probe(os.fsencode(p), ord(","), C.byref(n), None) == L.LDW_ERR_ARG and "separator" in L.lib().ldw_last_error().decode()
    assert IO.tsv_probe(p) == (3, False) and IO.tsv_probe(g, " ") == (5, True)
    with pytest.raises(FileNotFoundError):
        IO.tsv_probe(tmp_path / "no_such_file")


def test_null_context_refusals():
    lib = L.lib()
    rows, slow, mask = C.c_int64(0), C.c_int64(0), C.c_uint32(0)
    msg = lambda: lib.ldw_last_error().decode()
    assert lib.ldw_tsv_read(None, b"x", 9, 3, 0, C.byref(rows), C.byref(slow), C.byref(mask)) == L.LDW_ERR_ARG and msg() == "null context"
    p, n, nc, st = C.c_void_p(0), C.c_int64(0), C.c_int32(0), C.c_int64(0)
    assert lib.ldw_tsv_columns(None, C.byref(p), C.byref(n), C.byref(nc), C.byref(st)) == L.LDW_ERR_ARG and msg() == "null context"
    d = np.zeros(4)
    assert lib.ldw_tsv_fetch(None, 0, L.ptr(d), 4, 0) == L.LDW_ERR_ARG and msg() == "null context"
    pos = np.arange(4, dtype=np.int32)
    assert lib.ldw_set_positions(None, L.ptr(pos), 4, 100.0) == L.LDW_ERR_ARG and msg() == "null context"
    assert lib.ldw_links_load(None, 1, 0, 1, 5, 4, 20000.0, 0, None) == L.LDW_ERR_ARG and msg() == "null context"
    assert lib.ldw_tsv_stats(None, L.ptr(np.zeros(10))) == L.LDW_ERR_ARG
    assert lib.ldw_tsv_set_variant(None, 0) == L.LDW_ERR_ARG


def test_reader_keyword(tmp_path):
    sr = tmp_path / "sr.tsv"
    sr.write_text("1\t100\t2300\t1\t1\t2200\t0.31\t4.5\t1\n")
    for bad in ("Pandas", "arrow", None, 1):
        with pytest.raises(ValueError, match="reader must be one of"):
            P.read_ShortRangeLinks(sr, reader=bad)
        with pytest.raises(ValueError, match="reader must be one of"):
            P.read_LongRangeLinks(sr, reader=bad)
        with pytest.raises(ValueError, match="reader must be one of"):
            P.make_gwes_plots(sr_links=str(sr), plt_folder=str(tmp_path / "PL"), reader=bad)
    import inspect
    for fn in (P.read_ShortRangeLinks, P.read_LongRangeLinks, P.make_gwes_plots):
        assert inspect.signature(fn).parameters["reader"].default == "pandas"
    df = P.read_ShortRangeLinks(sr)            # the default route needs no device
    assert list(df.columns) == P.SR_COLS and df["srp_max"].tolist() == [4.5]
    with pytest.raises(ValueError, match="kind must be one of"):
        IO.read_links_native(sr, "tsv")
    with pytest.raises(ValueError, match='to must be'):
        IO.read_links_native(sr, "sr", to="numpy")
    with pytest.raises(ValueError, match="needs the engine"):
        IO.read_links_native(sr, "sr", to="device")
    sp = tmp_path / "sp3.txt"
    sp.write_text("1 2 3\n")
    with pytest.raises(ValueError, match="4 or 5 space-separated columns"):
        IO.table_shape(sp, "spydrpick")
    import ldweaver_amd
    assert ldweaver_amd.read_links_native is IO.read_links_native


def test_file_keywords_are_checked_before_any_device_work():
    with pytest.raises(ValueError, match="go with lr_links_path"):
        LR.genomewide_LDMap(None, sr_links_path="sr.tsv")
    with pytest.raises(ValueError, match="go with lr_links_path"):
        LR.analyse_long_range_links(None, sr_links_path="sr.tsv")
    with pytest.raises(ValueError, match="not sr_links"):
        LR.analyse_long_range_links(None, sr_links=pd.DataFrame(), lr_links_path="lr.tsv")
    with pytest.raises(ValueError, match="snp_dat and sr_links are needed"):
        LR.analyse_long_range_links(None)
