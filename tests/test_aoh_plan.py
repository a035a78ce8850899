"""The plain-C++ part of the two-phase form of AC over Huffman (weath3rb0i_amd/csrc/w3_aoh_plan.h: the bit-string helpers k_aoh_pack,
k_aoh_predict and k_aoh_coder share, and the layout / batch plan of the host) on the CPU: tests/host/aoh_plan.cpp packs seeded random
blocks under seeded random canonical tables, takes every step's (context, bit) back out and compares with a literal restatement of the
driver's loop; and checks the plan's offsets, batches, budget, block cap and 64-bit arithmetic."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "aoh_plan.cpp")
HDR = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_aoh_plan.h")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_aoh_plan_and_bit_strings(tmp_path):
    exe = str(tmp_path / "aoh_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert "aoh plan ok" in r.stdout


def _run_mutant(tmp_path, name, old, new):
    src = open(HDR, encoding="utf-8").read()
    bad = src.replace(old, new)
    assert bad != src
    hdr = tmp_path / (name + ".h")
    hdr.write_text(bad, encoding="utf-8")
    harness = open(SRC, encoding="utf-8").read().replace('"../../weath3rb0i_amd/csrc/w3_aoh_plan.h"', '"%s"' % str(hdr))
    p = tmp_path / (name + ".cpp")
    p.write_text(harness, encoding="utf-8")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, str(p)])
    return subprocess.run([exe, "50"], capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_harness_catches_codes_packed_lsb_first(tmp_path):
    """aoh_put_code patched to write every code's LAST bit first must fail the comparison with the driver's loop — otherwise the test
    above proves nothing about the bit order."""
    r = _run_mutant(tmp_path, "lsb_first", "if (len == 0u) return;",
                    "if (len == 0u) return; { uint32_t r = 0u; for (uint32_t i = 0u; i < len; i++) r |= ((code >> i) & 1u) << (len - 1u - i); code = r; }")
    assert r.returncode != 0 and "FAIL" in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_harness_catches_a_context_that_includes_the_coded_bit(tmp_path):
    """aoh_step_ctx shifted by one (the context would hold the bit being coded) must fail."""
    r = _run_mutant(tmp_path, "ctx_off_by_one", "(uint32_t)(window >> (8u - ((uint32_t)t & 7u))) & ctx_mask", "(uint32_t)(window >> (7u - ((uint32_t)t & 7u))) & ctx_mask")
    assert r.returncode != 0 and "FAIL" in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_harness_catches_a_plan_that_ignores_the_block_cap(tmp_path):
    r = _run_mutant(tmp_path, "no_cap", "(max_blocks && cur.count >= max_blocks)", "false")
    assert r.returncode != 0 and "FAIL" in r.stderr
