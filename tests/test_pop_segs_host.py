"""The popcount segment tables of a weighting and the rule that picks a form of the exact pair sums (ldweaver_amd/csrc/ldw_pairs.h: build_pop_segs,
choose_pair_form) checked on the HOST: the header is one source for prepare_apx_weights, for launch_pair_sums and for tests/host/pop_segs_check.cpp, which
compares both with hand-worked values — the tables on eight small weightings (word and class borders, zero runs, bit 31 of wbeg, the placeholder record),
the rule at each of its gates from both sides.  No GPU, no oracle: g++ only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pop_segs_and_form_rule_on_the_host(tmp_path):
    exe = str(tmp_path / "pop_segs_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "pop_segs_check.cpp")], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FAIL" not in out.stdout, out.stdout
    m = re.search(r"segs (\d+) forms (\d+) failures (\d+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) == 8 and int(m.group(2)) == 34 and int(m.group(3)) == 0
