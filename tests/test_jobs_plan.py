"""The decisions of the submit / wait job machinery (weath3rb0i_amd/csrc/w3_jobs.h: how many calls are kept in flight and how, which
slot a call takes, what a call's status words ask for) on the CPU: tests/host/jobs_plan.cpp compares them, on the edges, on seeded random
inputs and on every combination of the status signals, with the inline forms w3_encode_submit, the host-buffer and sharded submits,
encode_core's retry loop and w3_encode_wait had, and checks depth bounds, refusals and slot preference on their own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "jobs_plan.cpp")
HDR = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_jobs.h")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


@needs_gxx
def test_plans_slots_and_status_actions(tmp_path):
    exe = str(tmp_path / "jobs_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "jobs plan ok" in r.stdout


def _run_mutant(tmp_path, name, *edits):
    src = open(HDR, encoding="utf-8").read()
    for old, new in edits:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    hdr = tmp_path / (name + ".h")
    hdr.write_text(src, encoding="utf-8")
    harness = open(SRC, encoding="utf-8").read().replace('"../../weath3rb0i_amd/csrc/w3_jobs.h"', '"%s"' % str(hdr))
    p = tmp_path / (name + ".cpp")
    p.write_text(harness, encoding="utf-8")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, str(p)])
    return subprocess.run([exe, "50"], capture_output=True, text=True, timeout=600)


@needs_gxx
def test_the_harness_catches_four_jobs_with_slot_leaves(tmp_path):
    """a job's event records are 32 bytes per input byte and slot leaf: two jobs at most, whatever the size"""
    r = _run_mutant(tmp_path, "slot_depth4", ("if (has_slot) p.depth = 2;", "if (false) p.depth = 2;"))
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_the_timeout_before_the_lane_order_mismatch(tmp_path):
    """streams predicted out of lane order can stall the coder: the call is coded again on the ballot rounds, not reported broken"""
    r = _run_mutant(tmp_path, "timeout_first", ("if (two_phase && s.order_fault()) return", "if (two_phase && s.order_fault() && !s.timeout()) return"))
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_a_slot_taken_without_looking(tmp_path):
    r = _run_mutant(tmp_path, "blind_slot", ("    if (busy[j])\n", "    if (false)\n"), ("    if (!busy[j]) p.slot = j;", "    p.slot = j;"))
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_a_refusal_that_counts_only_the_slots_below_the_depth(tmp_path):
    """a call of another size may hold a slot beyond this call's depth: it still counts as in flight"""
    r = _run_mutant(tmp_path, "count_below_depth", ("for (int k = 0; k < n_slots; k++) p.in_flight += busy[k] != 0;",
                                                     "for (int k = 0; k < depth && k < n_slots; k++) p.in_flight += busy[k] != 0;"))
    assert r.returncode != 0 and "FAIL" in r.stderr
