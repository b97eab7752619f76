"""The layouts of the per-slot device buffers of a block's launch chain (ldweaver_amd/csrc/ldw_slots.h) checked on the HOST: the header is one source
for the engine and for tests/host/slot_layout_check.cpp, which lays the five buffers out for the smallest block, ragged sides, a from side without
one-row SNPs, spans of 2 and of LDW_SPAN_MAX segments and the C4 / C5 item shapes, and checks that the arrays are disjoint, aligned and inside the
reserved byte count, that each zeroed range is exactly the arrays it is stated for, that no buffer shrinks when a dimension grows, and that the
geometry reserve_slot_buffers sizes the buffers for covers the benchmark's items.  No GPU, no oracle: g++ only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_slot_layouts_on_the_host(tmp_path):
    exe = str(tmp_path / "slot_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "slot_layout_check.cpp")], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FAIL" not in out.stdout, out.stdout
    m = re.search(r"geometries (\d+)\s+failures (\d+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) >= 9 and int(m.group(2)) == 0
    assert len(re.findall(r"reserved ahead", out.stdout)) >= 3      # the C4 diagonal, the C4 span and the C5 shape against the ahead-of-time reserve
