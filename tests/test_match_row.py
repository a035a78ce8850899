"""The match-model leaf's byte-boundary work as k_decode_spec<.., MATCH>'s row of sixteen lanes compiles it
(weath3rb0i_amd/csrc/w3_match_spec_plan.h: plain C++, host and device) on the CPU: tests/host/match_row.cpp walks blocks of every size
1..40 and the directed inputs with sixteen simulated lanes against the serial match_advance, each block's output in a heap buffer of
exactly its size, every byte index asserted inside [0, known) — plainly, as a stand-alone program under -fsanitize=undefined,address, and
with headers wrong in one behaviour each, which the harness must catch."""
import os
import shutil
import subprocess
import zlib

import pytest

from tests import match_ref as mt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "match_row.cpp")
CSRC = os.path.join(ROOT, "weath3rb0i_amd", "csrc")
HDR = os.path.join(CSRC, "w3_match_spec_plan.h")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


def _run(exe):
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


@needs_gxx
def test_the_row_equals_the_serial_form(tmp_path):
    exe = str(tmp_path / "match_row")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    r = _run(exe)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "match row ok" in r.stdout
    # the program's directed inputs are match_ref.DIRECTED's, byte for byte
    seen = {}
    for line in r.stdout.splitlines():
        if line.startswith("input "):
            _, name, n, crc = line.split()
            seen[name] = (int(n), int(crc, 16))
    assert seen == {name: (len(x), zlib.crc32(x)) for name, x in mt.DIRECTED.items()}


@needs_gxx
def test_no_load_leaves_the_known_bytes_and_nothing_is_undefined(tmp_path):
    """the stand-alone program under both sanitizers: a load outside a block's heap buffer, a shift by too much or an overflow ends it"""
    exe = str(tmp_path / "match_row_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover", "-o", exe, SRC])
    r = _run(exe)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "match row ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def _run_mutant(tmp_path, name, old, new):
    src = open(HDR, encoding="utf-8").read()
    assert src.count(old) == 1, old
    inc = '#include "w3_match_plan.h"'
    assert src.count(inc) == 1
    hdr = tmp_path / (name + ".h")
    hdr.write_text(src.replace(old, new).replace(inc, '#include "%s"' % os.path.join(CSRC, "w3_match_plan.h")), encoding="utf-8")
    harness = open(SRC, encoding="utf-8").read()
    inc = '"../../weath3rb0i_amd/csrc/w3_match_spec_plan.h"'
    assert harness.count(inc) == 1
    p = tmp_path / (name + ".cpp")
    p.write_text(harness.replace(inc, '"%s"' % str(hdr)), encoding="utf-8")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, str(p)])
    return _run(exe)


@needs_gxx
def test_the_harness_catches_selection_by_the_high_nibble(tmp_path):
    r = _run_mutant(tmp_path, "select_high", "return r == (byte & 15u);", "return r == (byte >> 4);")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_a_window_shifted_by_one_byte(tmp_path):
    """the candidate-side window shifted by one byte"""
    r = _run_mutant(tmp_path, "window_off_by_one", "need_w ? end - 1u - s : ct;", "need_w ? end - s : ct;")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_rolling_words_that_drop_a_byte(tmp_path):
    r = _run_mutant(tmp_path, "push_drops", "n.w[2] = (n.w[2] << 8) | (n.w[1] >> 56);", "n.w[2] = (n.w[2] << 8) | (n.w[1] >> 48);")
    assert r.returncode != 0 and "FAIL" in r.stderr
