"""The parallel context statistics export (weath3rb0i_amd/csrc/w3_export.h) on the CPU: count, apply and replay per epoch driven as loops
over the 64 lanes of a wavefront by tests/host/export_lanes.cpp and compared there with a literal restatement of ordern.rs:26-44 and
counter.rs:20-26 (which never calls the code under test): the table, that D is left zeroed, that `replays` is the number of (context,
epoch) pairs in which the literal replay halves and at most 8 n / 32767, and that `halvings` is the replay's count.  The harness answers
"ok replays=.. halvings=.. epochs=.. nonzero=.. fold=.." only when all of that holds; what the inputs are meant to reach is asserted
here."""
import os
import re
import shutil
import subprocess

import pytest

from weath3rb0i_amd import _lib as L
from tests import export_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "export_lanes.cpp")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")

# the blob: markov_text(300000) | lcg_text(300000) | markov_text(70000)
D_IN, E_IN, F_IN = "blob:0:300000", "blob:300000:300000", "blob:600000:70000"
# id -> (input, bits, align, halvings, contexts that halve): inputs A - F of the issue (B: p = 0 .. 3 bytes 0xFF in front)
INPUTS = {"A": ("ffz:0:20000", 4, 0, 3, 1), "B0": ("ffz:0:65600", 3, 3, 8, 8), "B1": ("ffz:1:65600", 3, 3, 8, 8),
          "B2": ("ffz:2:65600", 3, 3, 8, 8), "B3": ("ffz:3:65600", 3, 3, 8, 8), "C": ("ffz:0:140000", 3, 3, 24, 8),
          "D": (D_IN, 6, 2, 11, 9), "E": (E_IN, 5, 0, 1, 1), "F": (F_IN, 11, 3, 0, 0)}
EPOCHS = (1024, 4096, 5120, 65536, 0)   # 0: the length rounded up to whole KiB (one epoch)
SHAPES = ((1, 0), (3, 3), (4, 0), (6, 2), (8, 7), (11, 3), (12, 5), (19, 3), (24, 3))
SHORT = (0, 1, 15, 16, 17, 1023, 1024, 1025)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "export", SRC)


answers = H.answers


def directed_cases():
    return [("exp %s %d %d %d %d" % (inp, bits, align, e, k % 16), key, e)
            for k, (key, (inp, bits, align, _, _)) in enumerate(INPUTS.items()) for e in EPOCHS]


@needs_gxx
def test_inputs_a_to_f_at_every_epoch_size(harness):
    cases = directed_cases()
    got = answers(harness, [c for c, _, _ in cases], "directed")
    for (case, key, e), g in zip(cases, got):
        _, _, _, halvings, contexts = INPUTS[key]
        assert g["halvings"] == halvings, (case, g)
        assert g["replays"] == halvings if e in (1024, 4096, 5120) else contexts <= g["replays"] <= halvings, (case, g)
        if e == 0:
            assert g["epochs"] == 1 and g["replays"] == contexts, (case, g)   # one epoch: one replay per context, however many halvings
    f = [g for (_, key, _), g in zip(cases, got) if key == "F"]
    assert all(g["replays"] == 0 and g["nonzero"] > 200 for g in f)


@needs_gxx
def test_input_b_puts_the_halving_on_the_epoch_edges(harness):
    """p bytes 0xFF before the zeros: every position's zero count reaches 65535 on byte p + 65534.  With epochs of 4,096 bytes that is the LAST byte
    of an epoch for p = 1, the FIRST of the next for p = 2, one byte inside for p = 0 and 3; cut into pieces there as well."""
    assert (1 + 65534) % 4096 == 4095 and (2 + 65534) % 4096 == 0
    cases = []
    for p in range(4):
        h = p + 65534
        for a in (0, 5, 16, 17):
            cases.append("exp ffz:%d:65600 3 3 4096 %d" % (p, a))
        for cuts in ((h,), (h + 1,), (h, h + 1), (4096, h)):
            cases.append("exp ffz:%d:65600 3 3 4096 3 %s" % (p, " ".join(map(str, cuts))))
    got = answers(harness, cases, "edges")
    assert all(g["halvings"] == 8 and g["replays"] == 8 for g in got)


@needs_gxx
def test_short_lengths_every_skew_between_inaccessible_pages(harness):
    """lengths 0 .. 1,059 around the chunk and row sizes.  Every pointer skew 0 .. 15 in a heap block that ends with the input (a byte read
    past it is caught by the sanitizer build below, a wrong byte before it by the table: other values sit there).  Between inaccessible
    pages: starting at a page start (16: skew 0 only; the history load of the first bytes must not reach back) and ending at a page end
    (17: the start skew follows the length, so every skew occurs over the lengths; a chunk loaded behind the end is a SIGSEGV)"""
    cases = []
    for n in list(SHORT) + list(range(2, 50)) + list(range(1000, 1060)):
        for a in list(range(16)) + [16, 17]:
            bits, align = SHAPES[(n + a) % (len(SHAPES) - 1)]   # (the 2^24 table: below, a few cases)
            cases.append("exp blob:%d:%d %d %d 1024 %d" % (7 * n + a, n, bits, align, a))
    for a in range(18):   # several rows and epochs, ragged at both ends
        cases.append("exp blob:%d:%d 11 3 2048 %d" % (a, 5000 + a, a))
    cases += ["exp blob:%d:%d 24 3 1024 %d" % (n, n, a) for n, a in ((1, 16), (17, 17), (1023, 5), (1025, 17))]
    got = answers(harness, cases, "short")
    assert got[0]["epochs"] == 0 and got[0]["nonzero"] == 0   # n == 0


@needs_gxx
def test_every_shape_and_pieces_cut_off_the_alignment_period(harness):
    """(bits, align) over the list, as one piece and as pieces cut at lengths that are no multiples of 2^align / 8 bytes (align > 3: the
    context depends on the absolute bit index, which the offset carries) and within four bytes of each other (the carried history)"""
    cases = []
    for bits, align in SHAPES:
        n = 40000 if bits == 24 else 70000
        cases.append("exp blob:1000:%d %d %d 4096 %d" % (n, bits, align, bits % 16))
        cases.append("exp blob:1000:%d %d %d 5120 %d 1 3 1030 1033 20001 20002" % (n, bits, align, (bits + 5) % 16))
        cases.append("exp blob:1000:%d %d %d 0 %d 7 4099" % (n, bits, align, (bits + 9) % 16))
    # sixteen contexts by bit index mod 16 that halve in bytes 131071 .. 131074, pieces cut there and off the 2-byte period
    cases.append("exp ffz:3:140000 5 4 4096 2 65537 131071 131073")
    cases.append("exp %s 6 2 65536 11 99999 100001 250003" % D_IN)
    got = answers(harness, cases, "shapes")
    assert got[-1]["halvings"] == 11 and got[-2]["halvings"] == 16
    whole, cut = got[0:-2:3], got[1:-2:3]
    assert [g["fold"] for g in whole] == [g["fold"] for g in cut]


@needs_gxx
def test_the_same_under_address_and_ub_sanitizers(harness, tmp_path):
    """A stand-alone sanitizer build of the harness (every piece lives in a heap block that ends with its last byte)."""
    san = H.SAN
    why = H.sanitizer_probe(tmp_path)
    if why:
        pytest.skip(why)
    exe = str(tmp_path / "export_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + san + ["-o", exe, SRC])   # (the harness itself must build)
    cases = [c for c, key, e in directed_cases() if e in (4096, 0) or key in ("A", "B1", "B2")]
    for n in SHORT + (33, 1040):
        for a in (0, 1, 7, 15):
            cases.append("exp blob:%d:%d 11 3 1024 %d" % (n, n, a))
            cases.append("exp blob:%d:%d 12 5 1024 %d 3 %d" % (n, n, a, n // 2 + 1))
    answers(harness, cases, "san", exe=exe)


def test_constants_and_struct_equal_the_header():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "w3hip.h"), encoding="utf-8").read()
    assert re.search(r"W3_OPT_EXPORT_EPOCH = (\d+)", hdr).group(1) == str(L.W3_OPT_EXPORT_EPOCH) == "15"
    m = re.search(r"typedef struct w3_export_profile \{(.*?)\} w3_export_profile;", hdr, re.S)
    names = re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert names == [n for n, _ in L.ExportProfile._fields_] and C.sizeof(L.ExportProfile) == 40
    for name in ("w3_export_counters_device", "w3_export_counters_staged", "w3_export_get_profile"):
        assert name in L.EXPORTS
