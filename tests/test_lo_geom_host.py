"""The low-limb geometry of the mixed-precision path (ldweaver_amd/csrc/ldw_lo_geom.h: lo_layout) checked on the HOST: the header is one source for
prep_block (PrepWork::tiles), for the test hook ldw_debug_lo_units and for tests/host/lo_geom_check.cpp, which compares it with hand-worked values on
three block shapes and with the arithmetic PrepWork::tiles had before it moved into the header on those and on 400 random shapes.  No GPU, no
oracle: g++ only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lo_layout_on_the_host(tmp_path):
    exe = str(tmp_path / "lo_geom_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "lo_geom_check.cpp")], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FAIL" not in out.stdout, out.stdout
    m = re.search(r"shapes (\d+)\s+random (\d+)\s+failures (\d+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) >= 3 and int(m.group(2)) == 400 and int(m.group(3)) == 0
