"""GPU: the chunk pass under ldw_tsv_read and ldw_links_grep: one file through both users at every cut, the too-long line in the
search, the shared pinned pair across interleaved calls, and a refusal in a later chunk followed by reuse of the engine."""
import numpy as np
import pytest

import links_ref as R
import network_ref as NR
from ldweaver_amd import _lib as L
from ldweaver_amd import engine as E
from test_network_gpu import _check, _rows

pytestmark = pytest.mark.gpu

NAMES = ("pos1", "pos2", "len", "ARACNE", "MI", "pos1_ann", "pos2_ann", "links")
NEEDLES = ["abc", "pbp2x", "dnaA", "lastrow", "absent"]


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """An annotated table of 40 rows (CR LF line ends, a blank line in front of the header and one among the rows, no final newline) and the numeric
    columns of the same rows without a header: (annotated path, its pandas frame, numeric path, its bytes)."""
    d = tmp_path_factory.mktemp("pass")
    r = _rows(120)
    rows = r[:30] + r[80:87] + r[-3:]          # the crafted rows 5, 17, 29 and 80..86 (slow cells among them) and the last one
    assert len(rows) == 40
    ann = ["", "\t".join(NAMES)] + ["\t".join(str(r[c]) for c in NAMES) for r in rows]
    ann.insert(23, "")
    num = ["\t".join(str(r[c]) for c in NAMES[:5]) for r in rows]
    num.insert(0, "")
    num.insert(21, "")
    a, n = d / "ann.tsv", d / "num.tsv"
    a.write_bytes("\r\n".join(ann).encode())
    n.write_bytes("\r\n".join(num).encode())
    tab = NR.read_annotated(a)
    assert len(tab) == 40
    return str(a), tab, str(n), n.read_bytes()


def _read(eng, path, chunk):
    rows, slow, ints = eng.tsv_read(path, "\t", 5, chunk)
    return [eng.tsv_fetch(k, rows) for k in range(5)], list(ints)


def _same_table(got, ref):
    return all(R.same_bits(a, b) for a, b in zip(got[0], ref[0])) and got[1] == ref[1]


@pytest.mark.parametrize("chunk", [64, 65, 4096, 0])
def test_one_file_through_both_passes_at_every_cut(engine, both, chunk):
    ann, tab, num, data = both
    assert _check(engine, ann, tab, NEEDLES, False, False, chunk) > 3
    _check(engine, ann, tab, NEEDLES, True, True, chunk)
    ref = R.parse(data, 5, b"\t")
    assert len(ref[0][0]) == 40
    assert _same_table(_read(engine, num, chunk), ref)
    if chunk:
        assert engine.tsv_stats()["chunks"] > (10 if chunk < 100 else 0) and engine.links_grep_stats()["chunks"] > (10 if chunk < 100 else 0)


@pytest.mark.parametrize("chunk", [4096, 0])
def test_a_line_over_one_mebibyte_is_refused_by_the_search(engine, tmp_path, chunk):
    """test_links_read_gpu.py's test of the reader, for the search: 4096-byte reads meet the line in the feeder, one read of the whole file in the kernel."""
    def table(name, line_bytes):
        fixed = "7\t9\t2\t1\t0.5\t%s\tgyrB:2\tnsXns"
        row = fixed % ("abc:" + "a" * (line_bytes - len(fixed % "abc:")))
        assert len(row) == line_bytes
        p = tmp_path / name
        p.write_text("\t".join(NAMES) + "\n" + "8\t9\t1\t1\t0.25\tabc:1\tdnaA:3\tnsXns\n" + row + "\n" + "9\t9\t1\t0\t0.125\tfolA:1\tabc:3\tsyXsy\n")
        return str(p)

    with pytest.raises(L.LdwError) as e:
        engine.links_grep(table("long.tsv", (1 << 20) + 8), ["abc"], False, False, chunk)
    msg = str(e.value)
    assert e.value.code == L.LDW_ERR_ARG and all(w in msg for w in ("ldw_links_grep:", "long.tsv", "line 3, column 1", "longer than")), msg
    g = engine.links_grep(table("fits.tsv", (1 << 20) - 16), ["abc"], False, False, chunk)
    assert g["row"].tolist() == [0, 1, 2] and g["num"][:, 4].tolist() == [0.25, 0.5, 0.125] and g["data_rows"] == 3
    assert len(g["pos1_ann"][1]) == (1 << 20) - 16 - len("7\t9\t2\t1\t0.5\t\tgyrB:2\tnsXns")


def _grep(eng, path, chunk):
    g = eng.links_grep(path, NEEDLES, False, False, chunk)
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in g.items()}


def test_interleaved_passes_share_one_pinned_pair(both):
    ann, _, num, _ = both
    with E.Engine(0) as fresh:
        want_read = _read(fresh, num, 0)
        want_pinned = fresh.tsv_stats()["pinned_bytes"]
    with E.Engine(0) as fresh:
        want_grep = _grep(fresh, ann, 64)
    assert want_pinned >= 2 * (64 << 20) and len(want_grep["row"]) > 3
    with E.Engine(0) as eng:
        assert _same_table(_read(eng, num, 64), want_read)
        small = eng.tsv_stats()["pinned_bytes"]
        assert 0 < small < want_pinned
        assert _grep(eng, ann, 4096) == want_grep
        assert _same_table(_read(eng, num, 0), want_read)
        assert _grep(eng, ann, 64) == want_grep
        assert eng.tsv_stats()["pinned_bytes"] == want_pinned          # the pair grows and never shrinks
        assert eng.host_trim() >= want_pinned and eng.tsv_stats()["pinned_bytes"] == 0
        assert _same_table(_read(eng, num, 64), want_read)             # ... and comes back on demand


def test_a_refusal_in_the_third_chunk_then_reuse(engine, both, tmp_path):
    """64-byte reads: the numeric file's chunks end at bytes 60, 126 and 192 (6-byte lines), the annotated file's at 48 (the header), 120 and 192 (18-byte
    rows); the bad cell lies at byte 146 of either.  Every exit of a pass waits for the stream, so the next call may refill the buffers."""
    ann, tab, num, data = both
    lines = ["1\t2\t3"] * 40
    lines[24] = "1\tx\t3"
    bad_num = tmp_path / "bad_num.tsv"
    bad_num.write_text("\n".join(lines) + "\n")
    assert 126 <= 24 * 6 + 2 < 192
    with pytest.raises(L.LdwError) as e:
        engine.tsv_read(bad_num, "\t", 3, 64)
    assert e.value.code == L.LDW_ERR_ARG and "ldw_tsv_read:" in str(e.value) and "bad_num.tsv: line 25, column 2: not a number" in str(e.value), str(e.value)
    assert _same_table(_read(engine, num, 64), R.parse(data, 5, b"\t"))

    header = "\t".join(NAMES)
    assert len(header) == 47
    rows = ["1\t2\t3\t1\t0.5\ta\tb\tc"] * 12
    rows[5] = "1\t2\t3\t1\tabc\ta\tb\tc"
    bad_ann = tmp_path / "bad_ann.tsv"
    bad_ann.write_text("\n".join([header] + rows) + "\n")
    assert 120 <= 48 + 5 * 18 + 8 < 192
    with pytest.raises(L.LdwError) as e:
        engine.links_grep(str(bad_ann), ["a"], False, False, 64)
    assert e.value.code == L.LDW_ERR_ARG and "ldw_links_grep:" in str(e.value) and "bad_ann.tsv: line 7, column 5: not a number" in str(e.value), str(e.value)
    _check(engine, ann, tab, NEEDLES, False, False, 64)
