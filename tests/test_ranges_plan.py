"""The plan of the random-access decode (weath3rb0i_amd/csrc/w3_ranges.h: distinct blocks and how far each is decoded, staging layout,
job order, the gather's pieces, the host variant's compact stream selection) on the CPU: tests/host/ranges_plan.cpp simulates the decode
the plan describes over thousands of seeded random cases and the edge cases, and compares it with the requested slices."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ranges_plan.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_ranges_plan_simulated_decode(tmp_path):
    exe = str(tmp_path / "ranges_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    r = subprocess.run([exe, "4000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "ranges plan ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_harness_catches_a_plan_that_decodes_only_to_the_range_start(tmp_path):
    """A planner that decodes a range's first block only as far as the range's own end inside it (not to the block end when the range
    runs on) must fail the simulation — otherwise the test above proves nothing about contiguous staging."""
    src = open(os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_ranges.h"), encoding="utf-8").read()
    bad = src.replace("emit(b, block_size);", "emit(b, b == merged[i].first ? block_size / 2 + 1 : block_size);")
    assert bad != src
    hdr = tmp_path / "w3_ranges.h"
    hdr.write_text(bad.replace('"../../include/w3hip.h"', '"%s"' % os.path.join(ROOT, "include", "w3hip.h")), encoding="utf-8")
    harness = open(SRC, encoding="utf-8").read().replace('"../../weath3rb0i_amd/csrc/w3_ranges.h"', '"%s"' % str(hdr))
    p = tmp_path / "ranges_bad.cpp"
    p.write_text(harness, encoding="utf-8")
    exe = str(tmp_path / "ranges_bad")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, str(p)])
    r = subprocess.run([exe, "200"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "FAIL" in r.stderr
