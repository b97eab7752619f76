"""GPU: the native FASTA feeder (``Engine.fasta_scan`` / ``Engine.fasta_encode``, csrc/ldw_fasta.cpp + the k_fasta_* kernels) against
numpy and the oracle: per-column counts for every chunking, the encoded states from the packed copy and from a second read of the file,
the reference's bundled sample, agreement of the two ``reader`` routes of the parsers, the error cases, and bounded host memory."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ldw_oracle as orc
from ldweaver_amd import _lib as L
from ldweaver_amd import extract
from ldweaver_amd.engine import Engine
from test_extract import _counts, _random_alignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SAMPLE = os.path.join(GOLDEN, "snp_sample.fa.gz")

pytestmark = pytest.mark.gpu


def _write(path, chars, width=70, gz=True, eol=b"\n"):
    data = []
    for i, row in enumerate(chars):
        data.append(f">seq{i} some description".encode() + eol)
        b = row.tobytes()
        w = width or len(b)
        for k in range(0, len(b), w):
            data.append(b[k:k + w] + eol)
    data = b"".join(data)
    if gz:
        data = gzip.compress(data)
    path.write_bytes(data)
    return str(path)


def _ref_states(chars, pos):
    return orc.encode_states([bytes(row[pos - 1]) for row in chars])


def test_counts_every_chunking(engine, tmp_path):
    rng = np.random.default_rng(11)
    chars = _random_alignment(rng, n=77, ltot=1531)
    path = _write(tmp_path / "a.fa.gz", chars, width=61)
    ref = _counts(chars)
    for chunk_rows in (1, 3, 64, 77):
        for io_bytes in (7, 0):
            for keep in (0, -1):
                names, ltot, counts = engine.fasta_scan(path, chunk_rows=chunk_rows, io_bytes=io_bytes, keep_bytes=keep)
                assert ltot == 1531 and names == [f"seq{i}" for i in range(77)]
                assert np.array_equal(counts, ref), (chunk_rows, io_bytes, keep)


@pytest.mark.parametrize("n,ltot,chunk_rows", [(77, 1531, 3), (130, 517, 64), (64, 333, 7), (200, 2049, 0), (1, 50, 1)])
def test_encode_packed_and_reread(engine, tmp_path, n, ltot, chunk_rows):
    """N not a multiple of 64, chunk boundaries inside the last 64-sequence tile; from the packed copy (keep) and by reading the file again."""
    rng = np.random.default_rng(n * 7 + ltot)
    chars = _random_alignment(rng, n=n, ltot=ltot)
    path = _write(tmp_path / "a.fa", chars, width=50, gz=False)
    for keep in (-1, 0):
        _, _, counts = engine.fasta_scan(path, chunk_rows=chunk_rows, keep_bytes=keep)
        pos = extract.snp_filter(counts, n, 0.5, 0.0) if n > 1 else np.arange(1, ltot + 1, 3, dtype=np.int32)
        assert len(pos) > 0
        tab = engine.fasta_encode(pos)
        ref = _ref_states(chars, pos)
        assert engine.L == len(pos) and engine.N == n
        assert np.array_equal(engine.get_alignment(), ref), keep
        assert np.array_equal(tab, orc.acgtn_table(ref))
        assert np.array_equal(engine.state_counts(), orc.acgtn_table(ref))
        # a second encode (the packed copy was released by the first): the file is read again, unsorted / repeated columns too
        pos2 = np.concatenate([pos[::-1], pos[:3]]).astype(np.int32)
        engine.fasta_encode(pos2)
        assert np.array_equal(engine.get_alignment(), _ref_states(chars, pos2))


def test_golden_sample(engine):
    g = np.load(os.path.join(GOLDEN, "snp_sample_states.npz"))
    golden = g["states"]                                    # (1268, 400)
    gcounts = np.stack([(golden == x).sum(axis=1) for x in range(5)])
    for keep in (-1, 0):
        names, ltot, counts = engine.fasta_scan(SAMPLE, chunk_rows=0 if keep else 37, keep_bytes=keep)
        assert (len(names), ltot) == (400, 1268)
        assert np.array_equal(counts, gcounts)
        engine.fasta_encode(np.arange(1, 1269, dtype=np.int32))
        assert np.array_equal(engine.get_alignment(), golden)
    pos = np.loadtxt(os.path.join(GOLDEN, "snp_sample.pos"), dtype=np.int64)
    assert len(pos) == 1268
    kept = extract.snp_filter(gcounts, 400)
    sd = extract.parse_fasta_SNP_alignment(SAMPLE, pos, engine=engine)
    assert np.array_equal(sd.POS, pos[kept - 1]) and np.array_equal(sd.states, golden[kept - 1])
    assert sd.g is None and len(sd.seq_names) == 400


def _same(a, b):
    assert a.seq_names == b.seq_names and a.g == b.g
    for f in ("POS", "states", "uqe", "r"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f


@pytest.mark.parametrize("layout", [dict(width=70, gz=True), dict(width=0, gz=False, eol=b"\r\n"), dict(width=9, gz=True)])
def test_parsers_agree(engine, tmp_path, layout):
    rng = np.random.default_rng(5)
    chars = _random_alignment(rng, n=93, ltot=811)
    path = _write(tmp_path / ("a.fa.gz" if layout["gz"] else "a.fa"), chars, **layout)
    pos = np.arange(811) * 5 + 3
    for method in ("default", "relaxed"):
        nat = extract.parse_fasta_alignment(path, method=method, engine=engine)
        py = extract.parse_fasta_alignment(path, method=method, engine=engine, reader="python")
        _same(nat, py)
        nat = extract.parse_fasta_SNP_alignment(path, pos, 0.2, 0.05, method=method, engine=engine)
        py = extract.parse_fasta_SNP_alignment(path, pos, 0.2, 0.05, method=method, engine=engine, reader="python")
        _same(nat, py)
    # the default engine of the parser (a context of its own)
    _same(extract.parse_fasta_alignment(path), extract.parse_fasta_alignment(path, reader="python"))


def test_errors(engine, tmp_path):
    ragged = tmp_path / "ragged.fa"
    ragged.write_bytes(b">a\nACGT\n>b\nACG\n")
    empty_rec = tmp_path / "empty.fa.gz"
    empty_rec.write_bytes(gzip.compress(b">a\nACGT\n>b\n>c\nACGT\n"))
    for p in (ragged, empty_rec):
        with pytest.raises(ValueError, match="different lengths"):
            extract.parse_fasta_alignment(str(p), engine=engine)
        with pytest.raises(ValueError, match="different lengths"):
            engine.fasta_scan(str(p))
    # a failed scan leaves no scan behind
    with pytest.raises(L.LdwError) as ei:
        engine.fasta_encode(np.array([1], dtype=np.int32))
    assert ei.value.code == L.LDW_ERR_STATE
    fresh = Engine(0)
    try:
        with pytest.raises(L.LdwError) as ei:
            fresh.fasta_encode(np.array([1, 2], dtype=np.int32))
        assert ei.value.code == L.LDW_ERR_STATE
        # rewritten between the passes, without the packed copy: the second read refuses it
        rng = np.random.default_rng(3)
        chars = _random_alignment(rng, n=20, ltot=300)
        path = _write(tmp_path / "r.fa", chars, gz=False)
        fresh.fasta_scan(path, keep_bytes=0)
        _write(tmp_path / "r.fa", chars[:19], gz=False)
        with pytest.raises(L.LdwError) as ei:
            fresh.fasta_encode(np.array([1, 2], dtype=np.int32))
        assert ei.value.code == L.LDW_ERR_STATE
        with pytest.raises(L.LdwError) as ei:          # a column outside 1..L_total
            fresh.fasta_scan(path, keep_bytes=0)
            fresh.fasta_encode(np.array([0], dtype=np.int32))
        assert ei.value.code == L.LDW_ERR_ARG
    finally:
        fresh.close()


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from ldweaver_amd.engine import Engine

def status():
    d = {}
    for line in open("/proc/self/status"):
        k, _, v = line.partition(":")
        if k in ("VmHWM", "VmRSS"):
            d[k] = int(v.split()[0]) * 1024
    return d

eng = Engine(0)
eng.fasta_scan(sys.argv[2])
eng.fasta_encode(np.array([1, 2], dtype=np.int32))
eng.get_alignment()
base = status()["VmRSS"]
names, ltot, counts = eng.fasta_scan(sys.argv[3])
pos = np.load(sys.argv[4])
eng.fasta_encode(pos)
peak = status()["VmHWM"]
np.savez(sys.argv[5], counts=counts, states=eng.get_alignment())
eng.close()
print(json.dumps(dict(growth=peak - base, n=len(names), ltot=ltot)))
"""


def test_bounded_host_memory(tmp_path):
    n, ltot = 2000, 210_000          # 420 MB of text, one line per record
    enc = orc._ENC
    rng = np.random.default_rng(9)
    base = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=ltot)]
    alt = np.frombuffer(b"ACGTN-acgt", dtype=np.uint8)
    var = rng.choice(ltot, size=4000, replace=False)      # the columns that vary: 10 % of the sequences differ there
    big = tmp_path / "big.fa"
    with open(big, "wb") as fh:
        for s in range(n):
            row = base.copy()
            m = var[rng.random(len(var)) < 0.1]
            row[m] = alt[rng.integers(0, len(alt), size=len(m))]
            fh.write(b">s%d\n" % s + row.tobytes() + b"\n")
    assert os.path.getsize(big) >= 400e6
    # numpy, in chunks of one record: the counts and, for the retained columns, the states
    counts = np.zeros((5, ltot), dtype=np.int64)
    cols = np.arange(ltot)
    with open(big, "rb") as fh:
        for line in fh:
            if line.startswith(b">"):
                continue
            counts[enc[np.frombuffer(line.rstrip(b"\n"), dtype=np.uint8)], cols] += 1
    pos = extract.snp_filter(counts, n)
    assert 1000 < len(pos) <= 4000
    states = np.empty((len(pos), n), dtype=np.uint8)
    with open(big, "rb") as fh:
        s = 0
        for line in fh:
            if not line.startswith(b">"):
                states[:, s] = enc[np.frombuffer(line, dtype=np.uint8)[pos - 1]]
                s += 1
    np.save(tmp_path / "pos.npy", pos)
    tiny = _write(tmp_path / "tiny.fa", np.frombuffer(b"ACGTACGT" * 4, dtype=np.uint8).reshape(4, 8), gz=False)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, tiny, str(big), str(tmp_path / "pos.npy"), str(tmp_path / "out.npz")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert (res["n"], res["ltot"]) == (n, ltot)
    assert res["growth"] <= 256 << 20, res          # the Python route holds the file's text at least twice (> 800 MB here)
    got = np.load(tmp_path / "out.npz")
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["states"], states)
