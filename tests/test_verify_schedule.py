"""The sampled verification's schedule (weath3rb0i_amd/csrc/w3_verify.h: which block each sample slot of each call re-predicts) on the
CPU: over any ceil(nb / S) consecutive calls every block is sampled — the short last block included —, no index reaches nb and no call
samples a block twice, for every block count up to 20,000 (the bound include/w3hip.h states for W3_OPT_VERIFY); and the same for
series of calls numbered as the library numbers them — shapes that alternate on one context, w3_encode_blocks' pieces."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "verify_schedule.cpp")
HDR = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_verify.h")

# the formula of rounds 1 - 4: slot s took block s * nb_full / S + (call mod floor(nb_full / S)), full-length blocks only
OLD_SCHEDULE = """static uint32_t sample_size(uint32_t nb, bool short_last, uint64_t bs, uint32_t v) {
    const uint64_t nb_full = nb - (short_last ? 1u : 0u);
    if (nb_full == 0) return 1u;
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(nb_full, std::max<uint64_t>(16u, nb_full * v / 256u)), std::max<uint64_t>(1u, v * (64ull << 20) / bs));
}
static uint32_t block_of(uint64_t call, uint32_t s, uint32_t nb, bool short_last, uint32_t S) {
    const uint32_t nb_full = nb - (short_last ? 1u : 0u);
    if (nb_full == 0) return 0u;
    const uint32_t gap = nb_full / S, rot = (uint32_t)(call % gap);
    return (uint32_t)((uint64_t)s * nb_full / S) + rot;
}
"""


# the numbering of rounds 1 - 4: one context-wide count of calls, one number per piece of a w3_encode_blocks call
OLD_NUMBERING = (("    return vc.next(n, bs);\n", "    (void)n; (void)bs;\n    return vc.clock++;\n"),
                 ("    (void)vc; (void)n_piece; (void)bs;\n    return host_call;\n", "    (void)host_call; (void)n_piece; (void)bs;\n    return vc.clock++;\n"))


def _compile(tmp_path, src, name):
    p = tmp_path / (name + ".cpp")
    p.write_text(src.replace('"../../weath3rb0i_amd/csrc/w3_verify.h"', '"%s"' % HDR), encoding="utf-8")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-o", exe, str(p)])
    return exe


def _old_source():
    src = open(SRC, encoding="utf-8").read()
    old = re.sub(r"static uint32_t sample_size\(.*?\n}\nstatic uint32_t block_of\(.*?\n}\n", lambda m: OLD_SCHEDULE, src, count=1, flags=re.S)
    assert old != src
    return old


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_every_block_is_sampled_within_the_stated_bound(tmp_path):
    exe = _compile(tmp_path, open(SRC, encoding="utf-8").read(), "verify_schedule")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-600:], r.stderr[-400:])
    assert "verify schedule ok" in r.stdout
    # the headline shape (1e9 B in 64 KiB blocks: 15,258 full blocks and a short one) and the shapes of the GPU tests
    for nb, short in ((15259, 1), (411, 1), (400, 0)):
        r = subprocess.run([exe, "report", str(nb), str(short), "65536" if nb > 1000 else "1024", "1"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "never sampled 0 of %d blocks" % nb in r.stdout, r.stdout
        assert ("short last block sampled" if short else "short last block none") in r.stdout, r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_harness_traps_the_round_4_schedule(tmp_path):
    """The same harness with the formula the kernels used until round 5 must fail — and report the blocks it never reached at the
    headline shape: 36 of the 15,258 full blocks and the short last one — otherwise the test above proves nothing."""
    exe = _compile(tmp_path, _old_source(), "verify_schedule_old")
    r = subprocess.run([exe, "report", "15259", "1", "65536", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "S 59 never sampled 37 of 15259 blocks, short last block never" in r.stdout, r.stdout
    for nb, missed in ((1559, 7), (3815, 7), (7630, 3), (1907, 3), (410, 10)):   # full blocks only: what the old formula counted
        r = subprocess.run([exe, "report", str(nb), "0", "65536", "1"], capture_output=True, text=True, timeout=120)
        assert "never sampled %d of %d blocks" % (missed, nb) in r.stdout, (nb, r.stdout)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 1 and r.stdout.startswith("FAIL"), r.stdout[-600:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_alternating_shapes_and_chunked_calls_sample_every_block(tmp_path):
    exe = _compile(tmp_path, open(SRC, encoding="utf-8").read(), "verify_series")
    r = subprocess.run([exe, "series"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "verify series ok" in r.stdout, (r.returncode, r.stdout[-600:], r.stderr[-400:])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_harness_traps_the_round_4_numbering(tmp_path):
    """With one context-wide count and a number per piece, two shapes that alternate while ceil(nb / S) is even each see only every
    other rotation, as do the pieces of a chunked call: the series check must fail."""
    src = open(SRC, encoding="utf-8").read()
    old = src
    for a, b in OLD_NUMBERING:
        assert a in old
        old = old.replace(a, b)
    exe = _compile(tmp_path, old, "verify_series_old")
    r = subprocess.run([exe, "series"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("FAIL series"), r.stdout[-600:]
