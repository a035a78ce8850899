"""The logistic mixer's step as the kernels compile it (weath3rb0i_amd/csrc/w3_mix_plan.h: plain C++, host and device) on the CPU:
tests/host/mix_step.cpp compares it, on extreme and seeded random (w, s, p, bit, rate) tuples, with a 64-bit restatement that spells the
floor divisions out — plainly, under -fsanitize=undefined (every product and sum must fit int32: the definition says so), and with
headers wrong in one behaviour each, which the harness must catch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "mix_step.cpp")
HDR = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_mix_plan.h")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


def _run(exe, arg="200"):
    return subprocess.run([exe, arg], capture_output=True, text=True, timeout=600)


@needs_gxx
def test_the_step_equals_its_64_bit_restatement(tmp_path):
    exe = str(tmp_path / "mix_step")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    r = _run(exe)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "mix step ok" in r.stdout


@needs_gxx
def test_the_step_is_free_of_undefined_behaviour(tmp_path):
    """signed overflow, shifts by too much: the sanitizer aborts the stand-alone program at the first one"""
    exe = str(tmp_path / "mix_step_ubsan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover", "-o", exe, SRC])
    r = _run(exe)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "mix step ok" in r.stdout and "runtime error" not in r.stderr


def _run_mutant(tmp_path, name, old, new):
    src = open(HDR, encoding="utf-8").read()
    assert src.count(old) == 1, old
    hdr = tmp_path / (name + ".h")
    hdr.write_text(src.replace(old, new), encoding="utf-8")
    harness = open(SRC, encoding="utf-8").read()
    inc = '"../../weath3rb0i_amd/csrc/w3_mix_plan.h"'
    assert harness.count(inc) == 1
    p = tmp_path / (name + ".cpp")
    p.write_text(harness.replace(inc, '"%s"' % str(hdr)), encoding="utf-8")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, str(p)])
    return _run(exe, "20")


@needs_gxx
def test_the_harness_catches_an_update_without_its_rounding_term(tmp_path):
    r = _run_mutant(tmp_path, "no_rounding", "(s * err + (1 << (rate - 1u))) >> rate", "(s * err) >> rate")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_a_truncating_division(tmp_path):
    r = _run_mutant(tmp_path, "truncating", "return (w * s) >> 8;", "return (w * s) / 256;")
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_the_harness_catches_a_clamp_at_2_to_the_20(tmp_path):
    r = _run_mutant(tmp_path, "clamp_2_20", "#define W3_MIX_WMAX ((1 << 20) - 1)", "#define W3_MIX_WMAX (1 << 20)")
    assert r.returncode != 0 and "FAIL" in r.stderr
