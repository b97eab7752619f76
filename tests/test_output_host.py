"""CPU: the port of the reference's alignment writers (tests/output_ref.py) pinned by hand on tiny inputs, and every argument error and
warning of ldweaver_amd.output raised before an engine is made."""
import warnings

import numpy as np
import pandas as pd
import pytest

import output_ref as R
from ldweaver_amd import output as O
from ldweaver_amd.snpdat import SnpDat

# 3 SNPs x 2 sequences: s1 = A G N, s2 = C T N
STATES = np.array([[0, 1], [2, 3], [4, 4]], dtype=np.uint8)
POS = np.array([100000, 7, 42], dtype=np.int32)
NAMES = ["s1", "s2"]


def _sd(names=NAMES, states=STATES):
    return SnpDat.from_states(states, POS, g=None, seq_names=names)


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine was made before the arguments were checked")
    monkeypatch.setattr(O, "Engine", boom)


def test_port_fasta_appends_and_writes_positions(tmp_path):
    aln, pos = tmp_path / "a.fa", tmp_path / "a.pos"
    R.snpdat_to_fa(STATES, POS, NAMES, str(aln), str(pos))
    assert aln.read_bytes() == b">s1\nAGN\n>s2\nCTN\n"
    assert pos.read_bytes() == b"100000\n7\n42\n"        # POS as it stands, integers
    R.snpdat_to_fa(STATES, POS, NAMES, str(aln), str(pos), pos=[42, 7])
    assert aln.read_bytes() == b">s1\nAGN\n>s2\nCTN\n>s1\nGN\n>s2\nTN\n"
    assert pos.read_bytes() == b"7\n42\n"                # overwritten, sorted


def test_port_tsv_header_has_no_leading_field(tmp_path):
    p = tmp_path / "a.tsv"
    R.snpdat_to_fa(STATES, POS, NAMES, str(p), format="tsv")
    assert p.read_bytes() == b"100000\t7\t42\ns1\tA\tG\tN\ns2\tC\tT\tN\n"
    R.snpdat_to_fa(STATES, POS, NAMES, str(p), pos=[7, 100000], format="tsv")
    assert p.read_bytes() == b"7\t100000\ns1\tG\tA\ns2\tT\tC\n"


def test_port_gwes_outliers_print_like_r(tmp_path):
    th = pd.DataFrame({"pos1": [100000.0, 7.0], "pos2": [42, 42], "len": [0.5, 99958.0], "ARACNE": [True, False], "srp": [1.0, 3.25],
                       "MI": [0.125, 1e-5]})
    R.write_output_for_gwes_explorer(STATES, POS, NAMES, th, str(tmp_path / "g"))
    assert (tmp_path / "g" / "snps.loci").read_bytes() == b"7\n42\n100000\n"
    assert (tmp_path / "g" / "snps.aln").read_bytes() == b">s1\nGNA\n>s2\nTNC\n"
    assert (tmp_path / "g" / "snps.outliers").read_text() == ("Pos_1 Pos_2 Distance Direct MI MI_wogaps\n"
                                                              "1e+05 42 0.5 1 1 0.125\n"
                                                              "7 42 99958 0 3.25 1e-05\n")
    assert O.outliers_table(th, "SR") == (tmp_path / "g" / "snps.outliers").read_text()


def test_outliers_srp_or_srp_max_and_lr():
    base = {"pos1": [100000], "pos2": [42], "len": [0.5], "ARACNE": [1], "MI": [0.25]}
    assert O.outliers_table(pd.DataFrame({**base, "srp_max": [4.5]}), "SR").splitlines()[1] == "1e+05 42 0.5 1 4.5 0.25"
    both = pd.DataFrame({**base, "srp_max": [4.5], "srp": [2.0]})
    assert O.outliers_table(both, "SR").splitlines()[1] == "1e+05 42 0.5 1 2 0.25"          # srp wins when present
    assert O.outliers_table(both, "LR").splitlines()[1] == "1e+05 42 0.5 1 0.25 0.25"
    with pytest.raises(ValueError, match="srp"):
        O.outliers_table(pd.DataFrame(base), "SR")
    assert O.outliers_table(pd.DataFrame(base), "LR").splitlines()[0] == "Pos_1 Pos_2 Distance Direct MI MI_wogaps"


def test_snpdat_to_fa_argument_errors(tmp_path, no_engine):
    aln, pos = str(tmp_path / "a.fa"), str(tmp_path / "a.pos")
    with pytest.raises(ValueError, match="requires a path for the pos file"):
        O.snpdat_to_fa(_sd(), aln)
    with pytest.warns(UserWarning, match="Format fa unsupported"):
        with pytest.raises(ValueError, match="requires a path for the pos file"):
            O.snpdat_to_fa(_sd(), aln, format="fa")
    with pytest.raises(ValueError, match="Duplicated entries found in pos"):
        O.snpdat_to_fa(_sd(), aln, pos, pos=[7, 42, 7])
    with pytest.raises(ValueError, match="pos= 8 cannot be extracted from snp.dat"):
        O.snpdat_to_fa(_sd(), aln, pos, pos=[7, 8])
    twice = SnpDat.from_states(STATES, np.array([7, 7, 42], dtype=np.int32), g=None, seq_names=NAMES)
    with pytest.raises(ValueError, match="pos= 7 cannot be extracted from snp.dat"):
        O.snpdat_to_fa(twice, aln, pos, pos=[7])
    with pytest.raises(ValueError, match="pos is empty"):
        O.snpdat_to_fa(_sd(), aln, pos, pos=[])
    with pytest.raises(ValueError, match="seq_names has 1 entries"):
        O.snpdat_to_fa(_sd(names=["s1"]), aln, pos)
    with pytest.raises(ValueError, match="seq_names has 0 entries"):
        O.snpdat_to_fa(_sd(names=[]), aln, format="tsv")
    with pytest.raises(ValueError, match="newline"):
        O.snpdat_to_fa(_sd(names=["s1", "a\nb"]), aln, pos)
    with pytest.raises(ValueError, match="needs the engine"):
        O.snpdat_to_fa(_sd(), aln, pos, alignment_resident=True)
    resident = SnpDat(states=None, POS=POS, g=None, uqe=np.zeros((3, 5)), r=np.zeros(3), seq_names=NAMES)
    with pytest.raises(ValueError, match="alignment_resident=True"):
        O.snpdat_to_fa(resident, aln, pos)
    assert not (tmp_path / "a.fa").exists() and not (tmp_path / "a.pos").exists()


def test_links_fasta_and_gwes_argument_errors(tmp_path, no_engine):
    with pytest.raises(ValueError, match="At least one links file must be provided"):
        O.generate_Links_SNPS_fasta(_sd(), str(tmp_path / "a.fa"), str(tmp_path / "a.pos"))
    with pytest.raises(ValueError, match="At least one links file must be provided"):
        R.generate_Links_SNPS_fasta(STATES, POS, NAMES, str(tmp_path / "a.fa"), str(tmp_path / "a.pos"))
    bad = tmp_path / "th.tsv"
    bad.write_text("pos1\tpos2\tMI\n7\t99\t0.5\n")
    with pytest.raises(ValueError, match="pos= 99 cannot be extracted"):
        O.generate_Links_SNPS_fasta(_sd(), str(tmp_path / "a.fa"), str(tmp_path / "a.pos"), sr_tophits_path=str(bad))
    th = pd.DataFrame({"pos1": [7], "pos2": [42], "len": [35.0], "ARACNE": [1], "MI": [0.5], "srp_max": [4.0]})
    g = str(tmp_path / "g")
    with pytest.raises(ValueError, match="links_type"):
        O.write_output_for_gwes_explorer(_sd(), th, g, links_type="XR")
    with pytest.raises(ValueError, match="tophits is empty"):
        O.write_output_for_gwes_explorer(_sd(), th.iloc[:0], g)
    with pytest.raises(ValueError, match="does not belong to exactly one SNP"):
        O.write_output_for_gwes_explorer(_sd(), th.assign(pos2=[43]), g)
    with pytest.raises(ValueError, match="seq_names has 3 entries"):
        O.write_output_for_gwes_explorer(_sd(names=["a", "b", "c"]), th, g)
    assert not (tmp_path / "g").exists()


def test_readers_keep_quotes_and_hashes(tmp_path):
    p = tmp_path / "ann.tsv"
    p.write_text('pos1\tpos2\tgene\n5\t9\t"x#1\n')
    for f in (O.read_TopHits, O.read_AnnotatedLinks):
        t = f(str(p))
        assert list(t.columns) == ["pos1", "pos2", "gene"] and t["gene"].tolist() == ['"x#1'] and t["pos1"].tolist() == [5]


def test_format_warning_falls_back_to_fasta(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(O, "_write", lambda sd, path, idx, names, fmt, append, eng, res: calls.append((fmt, append, idx.tolist())))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        O.snpdat_to_fa(_sd(), str(tmp_path / "a.fa"), str(tmp_path / "a.pos"), pos=[42, 100000], format="phylip")
    assert any(issubclass(x.category, UserWarning) and "phylip" in str(x.message) for x in w)
    assert calls == [(0, True, [2, 0])]
    assert (tmp_path / "a.pos").read_text() == "42\n100000\n"
