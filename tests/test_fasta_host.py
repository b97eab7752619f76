"""CPU: the native FASTA reader (csrc/ldw_fasta.cpp) through ``ldw_fasta_probe`` — no context, no GPU — against ``snpdat.read_fasta`` on
every layout the Python reader reads consistently, the reference's bundled sample, and the malformed inputs."""
import ctypes as C
import gzip
import os
import sys

import numpy as np
import pytest

from ldweaver_amd import _lib as L
from ldweaver_amd.extract import fasta_probe
from ldweaver_amd.snpdat import read_fasta

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMPLE = os.path.join(GOLDEN, "snp_sample.fa.gz")


def _chars(rng, n, ltot, alphabet=b"ACGTacgtNn-RYKMSWBDHV"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rng.integers(0, len(a), size=(n, ltot))]


def _fasta_bytes(names, chars, width=60, eol=b"\n", blank=False, desc=False):
    out = []
    for nm, row in zip(names, chars):
        out.append(b">" + nm.encode() + (b" some description\twith tabs" if desc else b"") + eol)
        if blank:
            out.append(eol)
        b = row.tobytes()
        w = width or len(b)
        for k in range(0, len(b), w):
            out.append(b[k:k + w] + eol)
            if blank and k % (3 * w) == 0:
                out.append(eol)
    return b"".join(out)


def _write(path, data, gz=False, members=1):
    if not gz:
        path.write_bytes(data)
        return
    cut = len(data) // 2 if members == 2 else len(data)
    with open(path, "wb") as fh:
        fh.write(gzip.compress(data[:cut]))
        if members == 2:
            fh.write(gzip.compress(data[cut:]))


LAYOUTS = [
    dict(width=1), dict(width=7), dict(width=60), dict(width=70), dict(width=0),     # 0: one line per record
    dict(width=60, eol=b"\r\n"), dict(width=7, blank=True), dict(width=70, desc=True),
    dict(width=13, eol=b"\r\n", blank=True, desc=True),
]


@pytest.mark.parametrize("io_bytes", [7, 4096, 0])
@pytest.mark.parametrize("kind", ["plain", "gz", "gz2"])
@pytest.mark.parametrize("li", range(len(LAYOUTS)))
def test_probe_matches_read_fasta(tmp_path, li, kind, io_bytes):
    rng = np.random.default_rng(100 + li)
    n, ltot = int(rng.integers(1, 9)), int(rng.integers(1, 400))
    chars = _chars(rng, n, ltot)
    names = [f"s{i}_{'x' * int(rng.integers(0, 20))}" for i in range(n)]
    path = tmp_path / ("aln.fa.gz" if kind != "plain" else "aln.fa")
    _write(path, _fasta_bytes(names, chars, **LAYOUTS[li]), gz=kind != "plain", members=2 if kind == "gz2" else 1)
    ref_names, ref_chars = read_fasta(str(path))
    assert ref_chars.shape == (n, ltot) and ref_names == names
    assert fasta_probe(str(path), io_bytes) == (ref_names, n, ltot)


def test_probe_spaces_and_header_forms(tmp_path):
    """Spaces inside sequence lines are kept (they count towards the length); a name is the first token after '>', "" if none."""
    data = b">a desc\nAC GT\n>  b\nAC-T \n>\nacgt \n>\tc\r\nNNNN \r\n"
    for io in (1, 7, 0):
        p = tmp_path / "s.fa"
        p.write_bytes(data)
        assert fasta_probe(str(p), io) == (["a", "b", "", "c"], 4, 5)
        names, chars = read_fasta(str(p))
        assert names == ["a", "b", "", "c"] and chars.shape == (4, 5)


def test_probe_skips_lines_before_the_first_header(tmp_path):
    p = tmp_path / "pre.fa"
    p.write_bytes(b"# comment\nACGT\n\n>a\nACG\n>b\nTTT\n")
    assert fasta_probe(str(p)) == (["a", "b"], 2, 3)


def test_probe_golden_sample():
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden
    finally:
        sys.path.remove(GOLDEN)
    names, seqs = make_golden.read_fasta_gz(SAMPLE)
    for io in (7, 0):
        got = fasta_probe(SAMPLE, io)
        assert got[1:] == (400, 1268) and got[0] == names
    assert len(seqs) == 400 and {len(s) for s in seqs} == {1268}


def _raw_probe(path):
    n, lt, nb = C.c_int64(), C.c_int64(), C.c_int64()
    rc = L.lib().ldw_fasta_probe(os.fsencode(path), 0, C.byref(n), C.byref(lt), None, 0, C.byref(nb))
    return rc, L.lib().ldw_last_error().decode()


@pytest.mark.parametrize("io_bytes", [3, 0])
def test_probe_errors(tmp_path, io_bytes):
    ragged = tmp_path / "ragged.fa.gz"
    _write(ragged, b">a\nACGT\n>b\nACG\n>c\nACGT\n", gz=True)
    empty_rec = tmp_path / "empty_rec.fa"
    empty_rec.write_bytes(b">a\nACGT\n>b\n>c\nACGT\n")
    empty_last = tmp_path / "empty_last.fa"
    empty_last.write_bytes(b">a\nACGT\n>b\nACGT\n>c\n\n")
    empty_first = tmp_path / "empty_first.fa"
    empty_first.write_bytes(b">a\n>b\nACGT\n")
    empty_file = tmp_path / "empty.fa"
    empty_file.write_bytes(b"")
    no_header = tmp_path / "noheader.fa"
    no_header.write_bytes(b"ACGT\nACGT\n")
    for p in (ragged, empty_rec, empty_last, empty_first):
        rc, msg = _raw_probe(p)
        assert rc == L.LDW_ERR_ARG and "sequences are of different lengths" in msg, (p, msg)
        with pytest.raises(ValueError, match="sequences are of different lengths"):
            fasta_probe(str(p), io_bytes)
    for p in (empty_file, no_header):
        rc, msg = _raw_probe(p)
        assert rc == L.LDW_ERR_ARG and "File does not contain any sequences!" in msg, (p, msg)
        with pytest.raises(ValueError, match="File does not contain any sequences!"):
            fasta_probe(str(p), io_bytes)
    missing = tmp_path / "missing.fa"
    rc, msg = _raw_probe(missing)
    assert rc != L.LDW_OK and "cannot open" in msg
    with pytest.raises(FileNotFoundError):
        fasta_probe(str(missing), io_bytes)


def test_probe_names_buffer_too_small(tmp_path):
    p = tmp_path / "a.fa"
    p.write_bytes(b">alpha\nAC\n>beta\nGT\n")
    n, lt, nb = C.c_int64(), C.c_int64(), C.c_int64()
    buf = C.create_string_buffer(4)
    assert L.lib().ldw_fasta_probe(os.fsencode(p), 0, C.byref(n), C.byref(lt), buf, 4, C.byref(nb)) == L.LDW_ERR_SIZE
    assert nb.value == len(b"alpha\0beta\0")
