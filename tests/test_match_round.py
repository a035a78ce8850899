"""The match-model leaf's index arithmetic as the kernels compile it (weath3rb0i_amd/csrc/w3_match_plan.h: plain C++, host and device) on
the CPU: tests/host/match_round.cpp walks blocks of every small size and several shapes in k_match_keys' round order over 64 simulated
lanes, and in the lane kernels' serial order, against the serial definition, asserting every byte index inside the block — one
wavefront's life over mixed blocks, then over inputs steered at the tag bookkeeping (the blocks where the tag is 1 again share no table
entry with the others) and one block of 70,000 bytes (entry positions above bit 16) — plainly, as a
stand-alone program under -fsanitize=undefined,address (each block in a heap buffer of exactly its size), and with headers wrong in one
behaviour each, which the harness must catch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "match_round.cpp")
HDR = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_match_plan.h")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


def _run(exe, arg="2"):
    return subprocess.run([exe, arg], capture_output=True, text=True, timeout=600)


@needs_gxx
def test_the_round_walk_equals_the_serial_definition(tmp_path):
    exe = str(tmp_path / "match_round")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    r = _run(exe)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "match round ok" in r.stdout


@needs_gxx
def test_no_load_leaves_the_block_and_nothing_is_undefined(tmp_path):
    """the stand-alone program under both sanitizers: a load outside a block's heap buffer, a shift by too much or an overflow ends it"""
    exe = str(tmp_path / "match_round_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover", "-o", exe, SRC])
    r = _run(exe)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "match round ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def _run_mutant(tmp_path, name, old, new):
    src = open(HDR, encoding="utf-8").read()
    assert src.count(old) == 1, old
    hdr = tmp_path / (name + ".h")
    hdr.write_text(src.replace(old, new), encoding="utf-8")
    harness = open(SRC, encoding="utf-8").read()
    inc = '"../../weath3rb0i_amd/csrc/w3_match_plan.h"'
    assert harness.count(inc) == 1
    p = tmp_path / (name + ".cpp")
    p.write_text(harness.replace(inc, '"%s"' % str(hdr)), encoding="utf-8")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, str(p)])
    return _run(exe, "1")


@needs_gxx
def test_the_harness_catches_a_round_without_the_lower_lane_rule(tmp_path):
    r = _run_mutant(tmp_path, "no_lower_lane", "return lower ? 63 - (int)__builtin_clzll(lower) : -1;", "(void)lower; return -1;")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_the_lowest_lane_as_candidate(tmp_path):
    r = _run_mutant(tmp_path, "lowest_lane", "return lower ? 63 - (int)__builtin_clzll(lower) : -1;", "return lower ? (int)__builtin_ctzll(lower) : -1;")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_the_lowest_lane_storing(tmp_path):
    r = _run_mutant(tmp_path, "lowest_writes", "return (M >> lane) >> 1 == 0ull;", "return (M & ((1ull << lane) - 1ull)) == 0ull;")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_a_tie_that_goes_to_the_long_context(tmp_path):
    r = _run_mutant(tmp_path, "tie_long", "return v_long > v_short;", "return v_long >= v_short;")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_a_compare_capped_at_31(tmp_path):
    r = _run_mutant(tmp_path, "cap_31", "MATCH_CAP = 32", "MATCH_CAP = 31")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_an_entry_taken_whatever_its_tag(tmp_path):
    """the tag comparison dropped from match_entry_pos: an earlier block's entry passes for a candidate"""
    r = _run_mutant(tmp_path, "no_tag_check", "return (entry >> 24) == tag ? entry & 0xFFFFFFu : 0u;", "(void)tag; return entry & 0xFFFFFFu;")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_a_position_field_of_16_bits(tmp_path):
    r = _run_mutant(tmp_path, "pos_16_bits", "return (entry >> 24) == tag ? entry & 0xFFFFFFu : 0u;", "return (entry >> 24) == tag ? entry & 0xFFFFu : 0u;")
    assert r.returncode != 0 and "FAIL" in r.stderr and "long block" in r.stderr
