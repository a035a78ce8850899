"""The plan of a CHECKED random-access decode (widen_to_whole_blocks, weath3rb0i_amd/csrc/w3_ranges.h) on the CPU: a CRC vouches for a
whole block, so every touched block is decoded to its true end.  tests/host/ranges_plan_whole.cpp checks the widened plan over thousands
of seeded random cases and the edge cases: block lengths, contiguous staging, the simulated decode + gather against the requested slices,
and that blocks, out_len and the pieces' destinations are the unwidened plan's."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ranges_plan_whole.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_whole_block_plan_simulated_decode(tmp_path):
    exe = str(tmp_path / "ranges_plan_whole")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    r = subprocess.run([exe, "4000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "whole-block plan ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_harness_catches_a_widening_that_forgets_the_piece_offsets(tmp_path):
    """A widening that moves the blocks in the staging buffer but leaves the pieces pointing at the old layout must fail the simulation."""
    src = open(os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_ranges.h"), encoding="utf-8").read()
    bad = src.replace("pc.src = p.bdst[k] + (pc.src - old_dst[k]);", "(void)k;")
    assert bad != src
    hdr = tmp_path / "w3_ranges.h"
    hdr.write_text(bad.replace('"../../include/w3hip.h"', '"%s"' % os.path.join(ROOT, "include", "w3hip.h")), encoding="utf-8")
    harness = open(SRC, encoding="utf-8").read().replace('"../../weath3rb0i_amd/csrc/w3_ranges.h"', '"%s"' % str(hdr))
    p = tmp_path / "whole_bad.cpp"
    p.write_text(harness, encoding="utf-8")
    exe = str(tmp_path / "whole_bad")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, str(p)])
    r = subprocess.run([exe, "200"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "FAIL" in r.stderr
