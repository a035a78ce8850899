"""The host's Counter-table arithmetic (weath3rb0i_amd/csrc/w3_tables_plan.h: the table-form rule, the sweep family's memory budget, the
batch planner of AC over Huffman's launches and the lanes of a batch) on the CPU: tests/host/tables_plan.cpp compares, on seeded random
inputs, every value the five places that apply the rule derive with what each derived when it spelled the rule out itself, and the
plans with the planning loops aoh_launch and aoh_spec_launch had; and checks the plans' coverage, budget, lane cap, table areas,
whole wavefronts and 64-bit products on their own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "tables_plan.cpp")
HDR = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_tables_plan.h")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_table_forms_and_batch_plans(tmp_path):
    exe = str(tmp_path / "tables_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "tables plan ok" in r.stdout


def _run_mutant(tmp_path, name, *edits):
    src = open(HDR, encoding="utf-8").read()
    for old, new in edits:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    hdr = tmp_path / (name + ".h")
    hdr.write_text(src, encoding="utf-8")
    harness = open(SRC, encoding="utf-8").read().replace('"../../weath3rb0i_amd/csrc/w3_tables_plan.h"', '"%s"' % str(hdr))
    p = tmp_path / (name + ".cpp")
    p.write_text(harness, encoding="utf-8")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, str(p)])
    return subprocess.run([exe, "50"], capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_harness_catches_a_planner_that_ignores_the_lane_cap(tmp_path):
    r = _run_mutant(tmp_path, "no_lane_cap", ("(!max_lanes || nb <= max_lanes)", "true"),
                    ("lanes_per_batch(budget, strides[c0], nb, max_lanes, 64)", "lanes_per_batch(budget, strides[c0], nb, 0, 64)"))
    assert r.returncode != 0 and "FAIL" in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_harness_catches_the_exact_map_on_a_tie(tmp_path):
    """direct on a tie is what every one of the five places did: a rule that takes the map there changes use_hash, strides and masks."""
    r = _run_mutant(tmp_path, "map_on_tie", ("t.use_hash = t.direct_bytes > t.hash_bytes;", "t.use_hash = t.direct_bytes >= t.hash_bytes;"))
    assert r.returncode != 0 and "FAIL" in r.stderr
