"""The host-only parts of a pass over a block list (ldweaver_amd/csrc/ldw_pass_plan.h) checked on the HOST: the header is one source for the engine
(ldw_mi_all_pairs) and for tests/host/pass_plan_check.cpp, which checks the block descriptor rule (each way out of range refused with "outside 1..",
the corners accepted), the plan (the spans of an 8 x 8 layout and of one with a ragged last block, shorter spans, no spans, what breaks a span, the
two caps at the segment that reaches them, items covering the blocks once and in order), the short-range pair count on the circle against brute
force, and the hand-over between three helper threads and the submitting thread: no item taken before its ring entry and its slot are free, every
item prepared once, a failure reported for the failed item and the ones behind it only, the lower of two failures, destruction with helpers
waiting.  No GPU, no oracle: g++ only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pass_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "pass_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "pass_plan_check.cpp")], check=True,
                   timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FAIL" not in out.stdout, out.stdout
    for group in ("descriptor: done", "plan: done", "short-range count:", "hand-over: done"):
        assert group in out.stdout, out.stdout
    m = re.search(r"checks (\d+)\s+failures (\d+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) >= 100 and int(m.group(2)) == 0
