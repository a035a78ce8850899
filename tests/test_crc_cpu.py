"""The CRC-32 arithmetic of weath3rb0i_amd/csrc/w3_crc.h on the CPU, against zlib.crc32: the bytewise definition, the per-lane piece of
k_crc32_slices driven as a loop over the 64 lanes of a wavefront plus the fold (every length 0 .. 2,100 at every start alignment, and the
lengths around the step, unroll and slice sizes), crc32_combine (also for lengths no buffer could hold), and — with the input flush
against an inaccessible page on either side — that not one byte outside the buffer is read.  tests/host/crc_lanes.cpp is the harness: the
test writes a blob and a case file, the harness prints one CRC per case."""
import os
import random
import shutil
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "crc_lanes.cpp")
HDR = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_crc.h")
BLOB_LEN = (1 << 21) + 4096
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


def compile_harness(out, src=SRC, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *extra, "-o", out, src])
    return out


@pytest.fixture(scope="module")
def blob():
    return random.Random(20261018).randbytes(BLOB_LEN)


@pytest.fixture(scope="module")
def harness(tmp_path_factory, blob):
    d = tmp_path_factory.mktemp("crc")
    (d / "blob").write_bytes(blob)
    return compile_harness(str(d / "crc_lanes")), str(d / "blob"), d


def answers(harness, cases, name="cases", exe=None, check=True):
    """run the harness over `cases` (lines) -> list of ints, one per answer"""
    exe0, blob_path, d = harness
    p = d / name
    p.write_text("\n".join(cases) + "\n")
    r = subprocess.run([exe or exe0, blob_path, str(p)], capture_output=True, text=True, timeout=600)
    if check:
        assert r.returncode == 0, (r.returncode, r.stdout[-200:], r.stderr[-800:])   # (-11: a read outside the buffer)
        return [int(x, 16) for x in r.stdout.split()]
    return r


def sweep_cases(blob, rng):
    """(b): every length 0 .. 2,100 at every start alignment 0 .. 15, and the lengths around the unrolled group, the slice and several slices"""
    cases, want = [], []
    for n in list(range(0, 2101)):
        for a in range(16):
            off = rng.randrange(0, len(blob) - n + 1)
            cases.append("wave %d %d %d" % (off, n, a))
            want.append(zlib.crc32(blob[off:off + n]))
    for n in (4095, 4096, 4097, 65535, 65536, 65537, 1048577):
        for a in (0, 1, 5, 15):
            off = rng.randrange(0, len(blob) - n + 1)
            cases.append("wave %d %d %d" % (off, n, a))
            want.append(zlib.crc32(blob[off:off + n]))
    return cases, want


def guard_cases(blob, rng):
    """(d): lengths 0 .. 2,100, the buffer starting at a page start and ending at a page end (the start alignment then follows the length)"""
    cases, want = [], []
    for n in range(0, 2101):
        for e in (0, 1):
            off = rng.randrange(0, len(blob) - n + 1)
            cases.append("guard %d %d %d" % (off, n, e))
            want.append(zlib.crc32(blob[off:off + n]))
    return cases, want


def test_crc32_ref_is_zlib(harness, blob):
    rng = random.Random(1)
    cases, want = ["known"], [0xCBF43926, 0]
    for _ in range(2000):
        n = rng.randrange(0, 5001)
        off = rng.randrange(0, len(blob) - n + 1)
        cases.append("ref %d %d" % (off, n))
        want.append(zlib.crc32(blob[off:off + n]))
    assert answers(harness, cases, "ref") == want


def test_the_lane_form_and_the_fold_are_zlib(harness, blob):
    cases, want = sweep_cases(blob, random.Random(2))
    got = answers(harness, cases, "wave")
    assert len(got) == len(want)
    bad = [(c, "%08x" % g, "%08x" % w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, bad[:5]


def test_crc32_combine(harness, blob):
    rng = random.Random(3)

    def comb(triples, name):
        return answers(harness, ["comb %x %x %d" % t for t in triples], name)

    # buffers that exist: |B| in 0 .. 70, 1023 .. 1025, 65,536
    tri, want = [], []
    for lb in list(range(0, 71)) + [1023, 1024, 1025, 65536]:
        la = rng.randrange(0, 3000)
        o = rng.randrange(0, len(blob) - la - lb + 1)
        A, B = blob[o:o + la], blob[o + la:o + la + lb]
        tri.append((zlib.crc32(A), zlib.crc32(B), lb))
        want.append(zlib.crc32(A + B))
    assert comb(tri, "comb1") == want
    # B all zeros, represented by its CRC alone: z[k] = crc of 2^k zero bytes by doubling, cross-checked against zlib at 2^20
    z = [zlib.crc32(b"\0")]
    for k in range(40):
        z.append(comb([(z[k], z[k], 1 << k)], "dbl")[0])
    assert z[20] == zlib.crc32(bytes(1 << 20)) and z[10] == zlib.crc32(bytes(1024))
    A = blob[:777]
    for big in ((1 << 31) + 5, (1 << 40) + 3):
        # crc(zeros(big)) and crc(A || zeros(big)), both assembled power of two by power of two
        zc, ac, first = 0, zlib.crc32(A), True
        for k in range(41):
            if big >> k & 1:
                zc = z[k] if first else comb([(zc, z[k], 1 << k)], "zc")[0]
                ac = comb([(ac, z[k], 1 << k)], "ac")[0]
                first = False
        assert comb([(zlib.crc32(A), zc, big)], "big") == [ac]


def test_no_byte_outside_the_buffer_is_read(harness, blob):
    cases, want = guard_cases(blob, random.Random(4))
    assert answers(harness, cases, "guard") == want


def test_the_harness_traps_a_tail_load_rounded_up_to_a_dword(harness, blob, tmp_path):
    """The same harness over a w3_crc.h whose bytewise loop runs to the next multiple of four bytes (what a dword load of the last bytes
    would touch) must die on the first buffer that ends at the page end — otherwise the test above proves nothing.  The loop mutated is
    the head's: a buffer that ends at a page end ends on a 16-byte boundary, so its ragged last bytes are never a tail — they are the
    head of a slice too short to hold an aligned chunk."""
    src = open(HDR, encoding="utf-8").read()
    assert src.count("i < pl.head;") == 1
    bad = src.replace("for (uint32_t i = 0; i < pl.head; i++)", "for (uint32_t i = 0; i < ((pl.head + 3u) & ~3u); i++)")
    assert bad != src
    (tmp_path / "w3_crc.h").write_text(bad, encoding="utf-8")
    h = open(SRC, encoding="utf-8").read().replace('"../../weath3rb0i_amd/csrc/w3_crc.h"', '"%s"' % str(tmp_path / "w3_crc.h"))
    (tmp_path / "crc_bad.cpp").write_text(h, encoding="utf-8")
    exe = compile_harness(str(tmp_path / "crc_bad"), str(tmp_path / "crc_bad.cpp"))
    cases, _ = guard_cases(blob, random.Random(4))
    r = answers(harness, cases, "guard_bad", exe=exe, check=False)
    assert r.returncode == -11, (r.returncode, r.stderr[-400:])


def test_the_same_under_address_and_ub_sanitizers(harness, blob, tmp_path):
    """A stand-alone sanitizer build of the harness (every `wave` case lives in a heap block that ends with its last byte)."""
    exe = str(tmp_path / "crc_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtime: " + r.stderr[-200:])
    rng = random.Random(5)
    cases, want = [], []
    for n in list(range(0, 2101, 3)) + [4095, 4096, 4097, 65535, 65536, 65537, 1048577]:
        a = rng.randrange(16)
        off = rng.randrange(0, len(blob) - n + 1)
        cases.append("wave %d %d %d" % (off, n, a))
        want.append(zlib.crc32(blob[off:off + n]))
    cases += ["ref 5 4000", "comb %x %x %d" % (1, 2, (1 << 40) + 3)]
    got = answers(harness, cases, "san", exe=exe)
    assert got[:len(want)] == want and got[len(want)] == zlib.crc32(blob[5:4005])
