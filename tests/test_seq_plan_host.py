"""The host-only parts of the sequence-level analyses (ldweaver_amd/csrc/ldw_seq_plan.h) checked on the HOST: the header is one source for the library
(ldw_nj.hip, ldw_pars.hip, ldw_lineage.hip, ldw_perm.hip) and for tests/host/seq_plan_check.cpp, which checks the SNP-index rule (empty lists, first and
last offender, 0 and L - 1 inside, pairs taken a before b), the label rule (-1 and C - 1 are labels, -2 and C are not, every label -1 gives P = 0), the
one neff summation against an independent long double loop on weights whose sum depends on order and precision, the distinct SNPs of one or two lists
and their slots, the budget hook (unset, "0", "-3", "7", text), the plan of ldw_links_stratified against brute force (the pieces partition the
positions, stay within a word and within one (label, V); the clusters' ranges; large and small jobs, 64 small clusters to a job; empty clusters in none)
and the order of ldw_links_permuted (stable by sequence within a label, v0 follows order0).  No GPU, no oracle: g++ only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_seq_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "seq_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "seq_plan_check.cpp")], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FAIL" not in out.stdout, out.stdout
    for group in ("indices: done", "labels: done", "neff: done", "distinct: done", "budget: done", "lin plan: done", "perm order: done"):
        assert group in out.stdout, out.stdout
    m = re.search(r"checks (\d+)\s+failures (\d+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) >= 100 and int(m.group(2)) == 0
