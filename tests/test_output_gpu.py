"""GPU: the alignment files of ldweaver_amd.output, rendered on the device (csrc/ldw_out.hip through ldw_write_alignment), byte-identical to the
literal port of tests/output_ref.py: the golden sample, shapes that break the 64 x 64 tiling, chunk budgets down to one record, the
keep_on_device route, the states after an MI pass, the links FASTA, GWESExplorer's three files, and a 100-MB alignment."""
import hashlib
import os
import time
import warnings

import numpy as np
import pandas as pd
import pytest

import output_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import extract
from ldweaver_amd import lr as LR
from ldweaver_amd import mi as MIH
from ldweaver_amd import output as O
from ldweaver_amd.engine import Engine
from ldweaver_amd.snpdat import CdsVar, SnpDat

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LUT = np.frombuffer(b"ACGTN", dtype=np.uint8)


def _render(states, idx, names, fmt=0):
    """numpy rendering of the same text (the second yardstick, and the one for large inputs)"""
    st = np.asarray(states)[np.asarray(idx)]
    out = []
    for s, n in enumerate(names):
        row = LUT[st[:, s]]
        if fmt == 0:
            out.append(b">" + n.encode() + b"\n" + row.tobytes() + b"\n")
        else:
            tab = np.empty(2 * len(row), dtype=np.uint8)
            tab[0::2], tab[1::2] = ord("\t"), row
            out.append(n.encode() + tab.tobytes() + b"\n")
    return b"".join(out)


def _names(n, rng):
    """short, empty, long (several waves of the header kernel) and spaced names"""
    out = []
    for i in range(n):
        kind = i % 5
        out.append(f"seq{i}" if kind < 2 else "" if kind == 2 and i % 3 else ("x" * int(rng.integers(60, 200)) + str(i)) if kind == 3
                   else f"isolate {i} / strain")
    return out


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sample_sd():
    g = np.load(os.path.join(GOLDEN, "snp_sample_states.npz"))
    names, n, _ = extract.fasta_probe(os.path.join(GOLDEN, "snp_sample.fa.gz"))
    assert n == g["states"].shape[1] == 400
    return SnpDat.from_states(g["states"], g["POS"], g=None, seq_names=names)


def test_golden_sample_fasta_tsv_and_subset(tmp_path, sample_sd):
    sd = sample_sd
    st, P, nm = sd.states, sd.POS, sd.seq_names
    assert st.shape == (1268, 400)
    for rep in range(2):   # the FASTA is appended to, the positions file overwritten
        O.snpdat_to_fa(sd, str(tmp_path / "a.fa"), str(tmp_path / "a.pos"))
        R.snpdat_to_fa(st, P, nm, str(tmp_path / "r.fa"), str(tmp_path / "r.pos"))
    assert (tmp_path / "a.fa").read_bytes() == (tmp_path / "r.fa").read_bytes() == _render(st, np.arange(1268), nm) * 2
    assert (tmp_path / "a.pos").read_bytes() == (tmp_path / "r.pos").read_bytes()
    O.snpdat_to_fa(sd, str(tmp_path / "a.tsv"), format="tsv")
    R.snpdat_to_fa(st, P, nm, str(tmp_path / "r.tsv"), format="tsv")
    assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "r.tsv").read_bytes()
    rng = np.random.default_rng(3)
    sub = rng.choice(P, size=333, replace=False)       # unsorted on the way in
    for fmt, ext in (("fasta", "fa"), ("tsv", "tsv")):
        O.snpdat_to_fa(sd, str(tmp_path / f"s.{ext}"), str(tmp_path / "s.pos"), pos=sub, format=fmt)
        R.snpdat_to_fa(st, P, nm, str(tmp_path / f"q.{ext}"), str(tmp_path / "q.pos"), pos=sub, format=fmt)
        assert (tmp_path / f"s.{ext}").read_bytes() == (tmp_path / f"q.{ext}").read_bytes(), fmt
    assert (tmp_path / "s.pos").read_bytes() == (tmp_path / "q.pos").read_bytes()
    assert (tmp_path / "s.pos").read_text().splitlines() == [str(x) for x in np.sort(sub)]


@pytest.mark.parametrize("Ls,N,k", [(130, 77, 70), (300, 200, 1), (90, 1, 90), (5, 1, 1), (200, 129, 191)])
def test_shapes_that_break_the_tiling(tmp_path, engine, Ls, N, k):
    """k and N not multiples of 64 (Npad != N), k = 1, N = 1; repeated rows in the selection"""
    rng = np.random.default_rng(Ls * 1000 + N)
    st = rng.integers(0, 5, size=(Ls, N), dtype=np.uint8)
    idx = rng.integers(0, Ls, size=k).astype(np.int32)
    names = _names(N, rng)
    engine.set_alignment(st)
    for fmt in (0, 1):
        p = str(tmp_path / f"o{fmt}")
        nb = engine.write_alignment(p, idx, names, format=fmt)
        want = _render(st, idx, names, fmt)
        assert nb == len(want) and open(p, "rb").read() == want, fmt
    sd = SnpDat.from_states(st, rng.permutation(np.arange(1, Ls + 1) * 3).astype(np.int32), g=None, seq_names=names)
    O.snpdat_to_fa(sd, str(tmp_path / "a.fa"), str(tmp_path / "a.pos"), engine=engine, alignment_resident=True)
    R.snpdat_to_fa(st, sd.POS, names, str(tmp_path / "r.fa"), str(tmp_path / "r.pos"))
    assert (tmp_path / "a.fa").read_bytes() == (tmp_path / "r.fa").read_bytes()
    O.snpdat_to_fa(sd, str(tmp_path / "a.tsv"), pos=sd.POS[idx[:1]], format="tsv", engine=engine, alignment_resident=True)
    R.snpdat_to_fa(st, sd.POS, names, str(tmp_path / "r.tsv"), pos=sd.POS[idx[:1]], format="tsv")
    assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "r.tsv").read_bytes()


def test_chunk_budgets(tmp_path, engine):
    """every sequence its own chunk (budget below one record), a budget that splits N unevenly, append after truncate"""
    rng = np.random.default_rng(11)
    st = rng.integers(0, 5, size=(700, 333), dtype=np.uint8)
    idx = rng.permutation(700)[:517].astype(np.int32)
    names = _names(333, rng)
    engine.set_alignment(st)
    for fmt in (0, 1):
        want = _render(st, idx, names, fmt)
        rec = len(want) // 333
        for budget in (1, int(rec * 3.5), 7 * rec + 13, 0):
            p = str(tmp_path / f"c{fmt}_{budget}")
            assert engine.write_alignment(p, idx, names, format=fmt, chunk_bytes=budget) == len(want)
            assert engine.write_alignment(p, idx, names, format=fmt, append=True, chunk_bytes=budget) == len(want)
            assert open(p, "rb").read() == want * 2, (fmt, budget)
    assert engine.host_trim() >= 0


def test_library_argument_errors(tmp_path, engine):
    st = np.zeros((10, 3), dtype=np.uint8)
    with Engine(0) as e:
        with pytest.raises(L.LdwError) as ei:
            e.write_alignment(str(tmp_path / "x"), [0], ["a", "b", "c"])
        assert ei.value.code == L.LDW_ERR_STATE
    engine.set_alignment(st)
    p = str(tmp_path / "x")
    for idx, names, what in (([10], ["a", "b", "c"], "outside"), ([-1], ["a", "b", "c"], "outside"), ([], ["a", "b", "c"], "k = 0"),
                             ([0], ["a", "b"], "2 names for 3"), ([0], ["a", "b", "c", "d"], "more than 3 names"),
                             ([0], ["a", "b\nc", "d"], "newline")):
        with pytest.raises(L.LdwError, match=what) as ei:
            engine.write_alignment(p, idx, names)
        assert ei.value.code == L.LDW_ERR_ARG
    assert not os.path.exists(p)      # nothing opened before the arguments passed
    with pytest.raises(L.LdwError, match="cannot open .*nodir") as ei:
        engine.write_alignment(str(tmp_path / "nodir" / "x"), [0], ["a", "b", "c"])
    assert ei.value.code == L.LDW_ERR_ARG


def test_keep_on_device_route_equals_host_states(tmp_path):
    fa = os.path.join(GOLDEN, "snp_sample.fa.gz")
    pos = np.array([int(x) for x in open(os.path.join(GOLDEN, "snp_sample.pos")).read().split()])
    host = extract.parse_fasta_SNP_alignment(fa, pos)
    assert host.states is not None
    sub = host.POS[::7]
    O.snpdat_to_fa(host, str(tmp_path / "h.fa"), str(tmp_path / "h.pos"))
    O.snpdat_to_fa(host, str(tmp_path / "h.tsv"), pos=sub, format="tsv")
    R.snpdat_to_fa(host.states, host.POS, host.seq_names, str(tmp_path / "r.fa"), str(tmp_path / "r.pos"))
    with Engine(0) as eng:
        dev = extract.parse_fasta_SNP_alignment(fa, pos, engine=eng, keep_on_device=True)
        assert dev.states is None
        O.snpdat_to_fa(dev, str(tmp_path / "d.fa"), str(tmp_path / "d.pos"), engine=eng, alignment_resident=True)
        O.snpdat_to_fa(dev, str(tmp_path / "d.tsv"), pos=sub, format="tsv", engine=eng, alignment_resident=True)
    for a, b in (("h.fa", "d.fa"), ("h.pos", "d.pos"), ("h.tsv", "d.tsv"), ("r.fa", "d.fa"), ("r.pos", "d.pos")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes(), (a, b)


def _gwes_files(folder):
    return [open(os.path.join(folder, f), "rb").read() for f in ("snps.loci", "snps.aln", "snps.outliers")]


def test_after_mi_pass_and_gwes_explorer(tmp_path, synth):
    """perform_MI_computation on the engine that holds the alignment leaves it intact; SR GWESExplorer files from the frame it returns, LR
    from analyse_long_range_links', each byte-identical to the port"""
    st, P = synth["states"], synth["POS"]
    names = [f"isolate_{i}" for i in range(st.shape[1])]
    sd = SnpDat.from_states(st, P, g=synth["g"], seq_names=names)
    cv = CdsVar(paint=synth["paint"], nclust=int(synth["paint"].max()))
    with Engine(0) as eng:
        eng.set_alignment(st)
        O.snpdat_to_fa(sd, str(tmp_path / "before.fa"), str(tmp_path / "before.pos"), engine=eng, alignment_resident=True)
        red = MIH.perform_MI_computation(sd, synth["hdw"], cv, lr_save_path=str(tmp_path / "lr.tsv"), sr_save_path=str(tmp_path / "sr.tsv"),
                                         plt_folder=str(tmp_path / "P"), sr_dist=50000, engine=eng, alignment_resident=True,
                                         verbose=False)   # (at 20 kb a cluster of the 512-SNP slice keeps too few links for the model)
        assert len(red) > 10 and "srp_max" in red.columns and "srp" not in red.columns
        O.snpdat_to_fa(sd, str(tmp_path / "after.fa"), str(tmp_path / "after.pos"), engine=eng, alignment_resident=True)
        O.snpdat_to_fa(sd, str(tmp_path / "after.tsv"), format="tsv", engine=eng, alignment_resident=True)
        sr_top = red.head(60)
        O.write_output_for_gwes_explorer(sd, sr_top, str(tmp_path / "gsr"), engine=eng, alignment_resident=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lr = LR.analyse_long_range_links(eng, sd, red, cv)["lr_links_red"]
        assert len(lr) > 0
        lr_top = lr.head(80)
        O.write_output_for_gwes_explorer(sd, lr_top, str(tmp_path / "glr"), links_type="LR", engine=eng, alignment_resident=True)
        O.write_output_for_gwes_explorer(sd, lr_top, str(tmp_path / "glr"), links_type="LR", engine=eng, alignment_resident=True)   # replaced
    R.snpdat_to_fa(st, P, names, str(tmp_path / "r.fa"), str(tmp_path / "r.pos"))
    R.snpdat_to_fa(st, P, names, str(tmp_path / "r.tsv"), format="tsv")
    assert (tmp_path / "before.fa").read_bytes() == (tmp_path / "after.fa").read_bytes() == (tmp_path / "r.fa").read_bytes()
    assert (tmp_path / "after.pos").read_bytes() == (tmp_path / "r.pos").read_bytes()
    assert (tmp_path / "after.tsv").read_bytes() == (tmp_path / "r.tsv").read_bytes()
    R.write_output_for_gwes_explorer(st, P, names, sr_top, str(tmp_path / "rsr"))
    R.write_output_for_gwes_explorer(st, P, names, lr_top, str(tmp_path / "rlr"), links_type="LR")
    assert _gwes_files(tmp_path / "gsr") == _gwes_files(tmp_path / "rsr")
    assert _gwes_files(tmp_path / "glr") == _gwes_files(tmp_path / "rlr")
    out = (tmp_path / "gsr" / "snps.outliers").read_text().splitlines()
    assert out[0] == "Pos_1 Pos_2 Distance Direct MI MI_wogaps" and len(out) == len(sr_top) + 1


def test_links_snps_fasta(tmp_path, sample_sd):
    sd = sample_sd
    rng = np.random.default_rng(5)
    P = sd.POS

    def links(n, extra):
        d = {"pos1": rng.choice(P, n), "pos2": rng.choice(P, n), "MI": rng.random(n)}
        d.update(extra)
        return pd.DataFrame(d)
    files = {}
    for key, extra in (("lr_tophits_path", {"gene": ["a#b"] * 12}), ("sr_tophits_path", {"srp_max": np.arange(9.0)[:9]}),
                       ("lr_annotated_links_path", {"note": ['"q'] * 15}), ("sr_annotated_links_path", {})):
        n = len(next(iter(extra.values()))) if extra else 20
        path = tmp_path / f"{key}.tsv"
        links(n, extra).to_csv(path, sep="\t", index=False, quoting=3)
        files[key] = str(path)
    O.generate_Links_SNPS_fasta(sd, str(tmp_path / "a.fa"), str(tmp_path / "a.pos"), **files)
    R.generate_Links_SNPS_fasta(sd.states, P, sd.seq_names, str(tmp_path / "r.fa"), str(tmp_path / "r.pos"), **files)
    assert (tmp_path / "a.fa").read_bytes() == (tmp_path / "r.fa").read_bytes()
    assert (tmp_path / "a.pos").read_bytes() == (tmp_path / "r.pos").read_bytes()
    one = {"sr_tophits_path": files["sr_tophits_path"]}
    O.generate_Links_SNPS_fasta(sd, str(tmp_path / "b.fa"), str(tmp_path / "b.pos"), **one)
    R.generate_Links_SNPS_fasta(sd.states, P, sd.seq_names, str(tmp_path / "q.fa"), str(tmp_path / "q.pos"), **one)
    assert (tmp_path / "b.fa").read_bytes() == (tmp_path / "q.fa").read_bytes()


def test_large_alignment_sha256(tmp_path, capfd, monkeypatch):
    """50 000 SNPs x 2 000 sequences (100 MB of FASTA) against numpy's rendering; wall time split into kernels, copies and write"""
    Ls, N = 50000, 2000
    rng = np.random.default_rng(2024)
    st = rng.integers(0, 5, size=(Ls, N), dtype=np.uint8)
    names = [f"sample_{i:05d}" for i in range(N)]
    monkeypatch.setenv("LDW_HOST_TIMING", "1")
    with Engine(0) as eng:
        eng.set_alignment(st)
        t0 = time.perf_counter()
        nb = eng.write_alignment(str(tmp_path / "big.fa"), np.arange(Ls, dtype=np.int32), names)
        wall = time.perf_counter() - t0
    err = capfd.readouterr().err
    line = [x for x in err.splitlines() if "write_alignment" in x]
    assert line, err[-2000:]
    h = hashlib.sha256()
    lut_t = LUT[st.T]                                           # (N, L) characters
    for s in range(N):
        h.update(b">" + names[s].encode() + b"\n")
        h.update(lut_t[s].tobytes())
        h.update(b"\n")
    assert nb == os.path.getsize(tmp_path / "big.fa") == N * (Ls + 2 + 12 + 1)
    with open(tmp_path / "big.fa", "rb") as fh:
        got = hashlib.sha256(fh.read()).hexdigest()
    assert got == h.hexdigest()
    with capfd.disabled():
        print(f"\n[write_alignment 50000 x 2000] {nb / 1e6:.1f} MB in {wall * 1e3:.1f} ms wall; {line[-1]}")
