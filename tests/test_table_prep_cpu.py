"""Table preparation (weath3rb0i_amd/csrc/w3_prep.h) on the CPU: the byte histogram's lane piece and StationaryModel::new's count + walk,
driven as loops over the 64 lanes of a wavefront by tests/host/prep_lanes.cpp and compared there with a byte loop and with the serial
Counter loop of counter.rs:20-25 (restated in the harness, which also reports where the halvings fall); with the input flush against an
inaccessible page on either side, that not one byte outside the buffer is read; and, through libw3hip.so without a GPU, that the
_from_counts builders are the builders of w3_huff_code_table and w3_huff_tables, error codes included."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests.synth import markov_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "prep_lanes.cpp")
HDR = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_prep.h")
T = L.W3_STAT_TILE
RAND_LEN = (1 << 20) + 4096
SKEW_LEN = 400000
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


def skewed(n, seed):
    """random bytes whose eight bit positions are one with eight different probabilities: the eight Counters halve at different bytes"""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=np.uint8)
    for i, pr in enumerate((0.02, 0.1, 0.3, 0.5, 0.7, 0.9, 0.97, 0.999)):
        out |= (rng.random(n) < pr).astype(np.uint8) << (7 - i)
    return out.tobytes()


@pytest.fixture(scope="module")
def blob():
    return random.Random(20261019).randbytes(RAND_LEN) + skewed(SKEW_LEN, 3)


@pytest.fixture(scope="module")
def harness(tmp_path_factory, blob):
    d = tmp_path_factory.mktemp("prep")
    (d / "blob").write_bytes(blob)
    exe = str(d / "prep_lanes")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    return exe, str(d / "blob"), d


def start(harness, cases, name, exe=None):
    exe0, blob_path, d = harness
    p = d / name
    p.write_text("\n".join(cases) + "\n")
    return subprocess.Popen([exe or exe0, blob_path, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def finish(proc, cases):
    out, err = proc.communicate(timeout=900)
    assert proc.returncode == 0, (proc.returncode, out[-300:], err[-800:])   # (-11: a read outside the buffer)
    lines = out.splitlines()
    assert len(lines) == len(cases)
    bad = [(c, ln[:200]) for c, ln in zip(cases, lines) if not ln.startswith("ok")]
    assert not bad, bad[:5]
    return lines


def answers(harness, cases, name="cases", exe=None):
    return finish(start(harness, cases, name, exe), cases)


def fields(line):
    """an `ok h=.. t=.. c=.. p0=..` answer -> dict of integer lists"""
    out = {}
    for k, v in re.findall(r"(\w+)=(\S*)", line):
        out[k] = [tuple(int(y) for y in x.split(":")) if ":" in x else int(x) for x in v.split(",")] if v else []
    return out


def fold(counts):
    """the harness's digest of 256 counts (FNV-1a over the 64-bit values)"""
    h = 1469598103934665603
    for c in counts:
        h = ((h ^ int(c)) * 1099511628211) % (1 << 64)
    return "ok %016x" % h


@needs_gxx
def test_histogram_lane_form_every_length_and_alignment(harness, blob):
    rng = random.Random(2)
    cases, want = [], []
    for n in list(range(0, 2101)):
        for a in range(16):
            off = rng.randrange(0, RAND_LEN - n + 1)
            cases.append("hist %d %d %d" % (off, n, a))
            want.append(fold(np.bincount(np.frombuffer(blob[off:off + n], dtype=np.uint8), minlength=256)))
    for n in (4095, 4096, 4097, 16383, 16384, 16385, 65537, 1048577):   # around a turn of 4 KiB, a workgroup's 16 KiB, several workgroups
        for a in (0, 1, 15):
            off = rng.randrange(0, RAND_LEN - n + 1)
            cases.append("hist %d %d %d" % (off, n, a))
            want.append(fold(np.bincount(np.frombuffer(blob[off:off + n], dtype=np.uint8), minlength=256)))
    assert answers(harness, cases, "hist") == want   # (the harness has compared with its own byte loop too)


@needs_gxx
def test_no_byte_outside_the_buffer_is_read(harness, blob):
    """the histogram's and the stationary count's lane pieces and the walk's tile loader, lengths 0 .. 2,100, the buffer starting at a page
    start and ending at a page end; every start alignment 0 .. 15 occurs at the page end (it follows the length)"""
    rng = random.Random(4)
    cases = []
    for n in range(0, 2101):
        for e in (0, 1):
            off = rng.randrange(0, RAND_LEN - n + 1)
            cases += ["histg %d %d %d" % (off, n, e), "statg %d %d %d" % (off, n, e)]
    for n in (4000, 4081, 4095, 4096):
        for e in (0, 1):
            cases += ["histg 5 %d %d" % (n, e), "statg 5 %d %d" % (n, e)]
    answers(harness, cases, "guard")


@needs_gxx
def test_the_harness_traps_a_chunk_loaded_behind_the_end(harness, tmp_path):
    """The same harness over a w3_prep.h that loads the chunks behind the input's end (a wave's turn is four KiB steps whatever is left of
    the input: those lanes must load nothing) must die on the first buffer that ends at the page end — otherwise the test above proves
    nothing.  An aligned 16-byte load cannot cross a page, so what the pages catch is a chunk too many; a byte too many inside a chunk
    is caught by the sanitizer build (past the end) and by the counts (before the start: other values sit there)."""
    src = open(HDR, encoding="utf-8").read()
    good = "vhi = w0 >= win.end ? 0u :"
    assert src.count(good) == 1
    (tmp_path / "w3_prep.h").write_text(src.replace(good, "vhi = w0 >= win.end ? 16u :"), encoding="utf-8")
    h = open(SRC, encoding="utf-8").read().replace('"../../weath3rb0i_amd/csrc/w3_prep.h"', '"%s"' % str(tmp_path / "w3_prep.h"))
    (tmp_path / "prep_bad.cpp").write_text(h, encoding="utf-8")
    exe = str(tmp_path / "prep_bad")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.dirname(SRC), "-o", exe, str(tmp_path / "prep_bad.cpp")])   # (-I: lanes_common.h)
    for case in ("histg 0 1000 1", "statg 0 1000 1"):
        p = start(harness, [case], "guard_bad", exe=exe)
        p.communicate(timeout=60)
        assert p.returncode == -11, (case, p.returncode)


@needs_gxx
def test_stationary_sizes_alignments_and_skewed_data(harness, blob):
    rng = random.Random(5)
    cases = []
    for n in (0, 1, T - 1, T, T + 1, 65534, 65535, 65536, 2 * T + 1, 64 * T - 1, 64 * T, 64 * T + 1):
        for a in (0, 1, 7, 15):
            cases.append("stat %d %d %d" % (rng.randrange(0, RAND_LEN - n + 1), n, a))
    first = len(cases)
    for a in (0, 3, 15):   # the skewed part of the blob: 5 to 11 halvings per position, at different bytes
        cases.append("stat %d %d %d" % (RAND_LEN, SKEW_LEN, a))
        cases.append("stat %d %d %d 100000 250000" % (RAND_LEN, SKEW_LEN, a))
        cases.append("stat %d %d %d %d" % (RAND_LEN, SKEW_LEN, a, 64 * T - a))
    lines = answers(harness, cases, "stat")
    f0 = fields(lines[0])
    assert f0["h"] == [0] * 8 and f0["t"] == [32768] * 8   # n == 0: eight fresh Counters
    f = fields(lines[first])
    assert min(f["h"]) >= 5 and len({tuple(f["p%d" % i]) for i in range(8)}) == 8, f["h"]
    # against the host function of the library (which an existing test pins to the oracle)
    for c, ln in zip(cases, lines):
        _, off, n = c.split()[:3]
        assert fields(ln)["t"] == w3.StationaryModel.new(blob[int(off):int(off) + int(n)]).table, c


@needs_gxx
def test_stationary_prefix_family_every_byte_offset_of_a_tile(harness):
    """k bytes 0xFF in front of 65,540 zero bytes, k = 0 .. 2T + 1: the first halving (the 65,535th zero) falls on byte k + 65,534, so every
    byte offset of a tile takes it; the same with the polarities swapped, so that c1 is the count that hits; each input also as two and
    three calls cut at that byte, behind it and at the tile edges around it.  Four processes: the serial loop is the slow part."""
    jobs = []
    for pol in (0, 1):
        for lo, hi, a in ((0, T // 2, 0), (T // 2 + 1, T - 1, 0), (T, T + T // 2, 5), (T + T // 2 + 1, 2 * T + 1, 11)):
            jobs.append(["pre %d %d %d 65540 %d" % (pol, lo, hi, a)])
    lines = []
    for k in range(0, len(jobs), 4):
        procs = [start(harness, c, "pre%d" % (k + j)) for j, c in enumerate(jobs[k:k + 4])]
        lines += [finish(p, c)[0] for p, c in zip(procs, jobs[k:k + 4])]
    for pol in (0, 1):
        got = [fields(ln) for ln in lines[4 * pol:4 * pol + 4]]
        assert sum(g["cases"][0] for g in got) == 2 * T + 2
        # k = 0 .. T - 1 at one alignment: T consecutive bytes, every residue mod T once
        assert got[0]["residues"][0] + got[1]["residues"][0] == T and got[0]["residues"][0] == T // 2 + 1


@needs_gxx
def test_stationary_halvings_at_batch_edges_in_short_tiles_and_eight_of_them(harness):
    last = 64 * T - 1   # window position of the last byte of a batch's last tile
    cases = ["runs 0 300000",          # zeros: halvings every 32,767 bytes from byte 65,534 on, 8 of them
             "runs 0 0 7 300000",      # 7 bytes 0xFF in front: the 7th halving on the LAST byte of tile 63, the last tile of the first batch
             "runs 0 0 8 300000",      # 8: on the FIRST byte of tile 64, the first tile of the next batch
             "runs 5 65535",           # the only halving on the last byte of a short last tile (tile 16 holds 4 bytes)
             "runs 0 0 3 65535",       # ... in a last tile of 2 bytes
             "runs 2 70000 70000 70000",
             "runs 9 0 300000"]        # ones: c1 is the count that hits
    f = [fields(ln) for ln in answers(harness, cases, "runs")]
    assert f[0]["h"] == [8] * 8 and f[6]["h"] == [8] * 8
    assert last in f[1]["p0"] and f[1]["p0"].index(last) == 6
    assert last + 1 in f[2]["p0"] and (last + 1) // T % 64 == 0 and last // T % 64 == 63
    assert f[3]["p0"] == [65539] and 65539 // T == 16 and (5 + 65535 - 1) == 65539      # the input's last byte
    assert f[4]["p0"] == [65537] and 65537 // T == 16 and (3 + 65535 - 1) == 65537
    assert f[5]["h"] == [3] * 8


@needs_gxx
def test_the_same_under_address_and_ub_sanitizers(harness, tmp_path):
    """A stand-alone sanitizer build of the harness (every input lives in a heap block that ends with its last byte)."""
    exe = str(tmp_path / "prep_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtime: " + r.stderr[-200:])
    rng = random.Random(6)
    cases = []
    for n in list(range(0, 2101, 7)) + [4095, 4096, 4097, 65537]:
        a, off = rng.randrange(16), rng.randrange(0, RAND_LEN - n + 1)
        cases += ["hist %d %d %d" % (off, n, a), "stat %d %d %d" % (off, n, a)]
    cases += ["stat %d %d 3 100000 250000" % (RAND_LEN, SKEW_LEN), "runs 0 0 7 300000", "runs 5 65535", "pre 0 0 8 65540 0", "pre 1 %d %d 65540 13" % (T - 3, T + 3)]
    answers(harness, cases, "san", exe=exe)


# ---- through libw3hip.so, no GPU ---------------------------------------------------------------------------------------------------
def inputs():
    rng = np.random.default_rng(8)
    return {"text": markov_text(60000, seed=1), "random": rng.integers(0, 256, 50000, dtype=np.uint8).tobytes(), "one": b"q" * 777,
            "two": b"ab" * 500, "few": bytes(rng.integers(0, 9, 3000, dtype=np.uint8))}


def counts_of(data):
    return np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256).astype(np.uint64)


def code_rc(lib, fn, *args):
    out = L.HuffCode()
    rc = fn(*args, C.byref(out))
    return rc, bytes(out)


def tables_rc(lib, fn, *args):
    out = L.HuffTable()
    rc = fn(*args, C.byref(out))
    return rc, bytes(out)


def test_from_counts_builders_are_the_builders():
    lib = L.load()
    seen = set()
    for name, data in inputs().items():
        a = np.frombuffer(data, dtype=np.uint8)
        c = counts_of(data)
        ap, cp = a.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)
        for size in range(7, 17):
            want = code_rc(lib, lib.w3_huff_code_table, ap, len(a), size)
            assert code_rc(lib, lib.w3_huff_code_from_counts, cp, size) == want, (name, size)
            seen.add(want[0])
            for rem in (7, 9, 12, 16):
                want = tables_rc(lib, lib.w3_huff_tables, ap, len(a), size, rem)
                assert tables_rc(lib, lib.w3_huff_tables_from_counts, cp, size, rem) == want, (name, size, rem)
                seen.add(want[0])
    assert seen == {L.W3_OK, L.W3_E_INVALID}   # (random data at a limit of 7: too small for 256 symbols)


def test_from_counts_error_codes_equal_the_buffer_forms():
    lib = L.load()
    data = inputs()["random"]
    a, c = np.frombuffer(data, dtype=np.uint8), counts_of(data)
    ap, cp = a.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)
    zero = np.zeros(256, dtype=np.uint64)
    zp = zero.ctypes.data_as(C.c_void_p)
    # a limit that is too small, no symbols, a size above 16 / above 32
    for size in (0, 1, 7, 17, 33, 255):
        assert code_rc(lib, lib.w3_huff_code_from_counts, cp, size)[0] == code_rc(lib, lib.w3_huff_code_table, ap, len(a), size)[0], size
        assert tables_rc(lib, lib.w3_huff_tables_from_counts, cp, size, 12)[0] == tables_rc(lib, lib.w3_huff_tables, ap, len(a), size, 12)[0] == L.W3_E_INVALID, size
        assert tables_rc(lib, lib.w3_huff_tables_from_counts, cp, 12, size)[0] == tables_rc(lib, lib.w3_huff_tables, ap, len(a), 12, size)[0], size
    assert code_rc(lib, lib.w3_huff_code_from_counts, cp, 7)[0] == L.W3_E_INVALID
    assert code_rc(lib, lib.w3_huff_code_from_counts, zp, 12)[0] == code_rc(lib, lib.w3_huff_code_table, None, 0, 12)[0] == L.W3_E_INVALID
    assert tables_rc(lib, lib.w3_huff_tables_from_counts, zp, 12, 12)[0] == tables_rc(lib, lib.w3_huff_tables, None, 0, 12, 12)[0] == L.W3_E_INVALID
    assert code_rc(lib, lib.w3_huff_code_from_counts, None, 12)[0] == L.W3_E_INVALID
    big = zero.copy()
    big[65], big[66] = 2**32, 5    # a count the reference's u32 could not hold
    bp = big.ctypes.data_as(C.c_void_p)
    assert code_rc(lib, lib.w3_huff_code_from_counts, bp, 12)[0] == L.W3_E_UNSUPPORTED
    assert tables_rc(lib, lib.w3_huff_tables_from_counts, bp, 12, 12)[0] == L.W3_E_UNSUPPORTED
    big[65] = 2**32 - 1
    assert code_rc(lib, lib.w3_huff_code_from_counts, bp, 12)[0] == L.W3_OK


def test_python_from_counts_and_the_error_they_raise():
    data = inputs()["text"]
    c = counts_of(data)
    assert bytes(w3.HuffCode.from_counts(c, 12).table) == bytes(w3.HuffCode.new(data, 12).table)
    assert bytes(w3.HuffHistory.from_counts(c, 12, 9).tables) == bytes(w3.HuffHistory.new(data, 12, 9).tables)
    rnd = counts_of(inputs()["random"])
    for f in (lambda: w3.HuffCode.from_counts(rnd, 7), lambda: w3.HuffHistory.from_counts(rnd, 7, 12), lambda: w3.HuffCode.from_counts(rnd[:100], 12)):
        with pytest.raises(w3.W3Error) as e:
            f()
        assert e.value.code == L.W3_E_INVALID


def test_header_constants_equal_their_python_mirrors():
    hdr = open(os.path.join(ROOT, "include", "w3hip.h"), encoding="utf-8").read()
    prep = open(HDR, encoding="utf-8").read()
    for name, val in (("W3_STAT_TILE", L.W3_STAT_TILE), ("W3_STAT_BATCH", L.W3_STAT_BATCH), ("W3_HIST_REP", L.W3_HIST_REP)):
        for text in (hdr, prep):
            m = re.findall(r"#define %s (\d+)u" % name, text)
            assert m == [str(val)], (name, m)
    assert T <= 32767 and T == 64 * 64
    want = [("hist_ms", 4), ("hist_sum_ms", 4), ("stat_count_ms", 4), ("stat_walk_ms", 4), ("halvings", 32), ("table", 16), ("counts", 2048)]
    assert [(n, C.sizeof(t)) for n, t in L.PrepProfile._fields_] == want and C.sizeof(L.PrepProfile) == 16 + 32 + 16 + 2048
    m = re.search(r"typedef struct w3_prep_profile \{(.*?)\} w3_prep_profile;", hdr, re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?[,;]", re.sub(r"/\*.*?\*/", "", m.group(1))) == [n for n, _ in want]
