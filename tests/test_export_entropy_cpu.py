"""The parallel context statistics export for OrderNEntropy leaves (weath3rb0i_amd/csrc/w3_export_entropy.h) on the CPU: the key stage,
keyed count, apply and keyed replay per epoch driven as loops over the 64 lanes of a wavefront by tests/host/export_entropy_lanes.cpp and
compared there with a literal restatement of ordern_entropy.rs:27-45 and counter.rs:20-26 over the oracle's History (which never calls the
code under test): the keys of every epoch, the table, that D is left zeroed, that `replays` is the number of (context, epoch) pairs in
which the literal run halves and at most 8 n / 32767, and that `halvings` is the literal's count.  The harness answers "ok ..." only when
all of that holds; what the inputs are meant to reach is asserted here.  The coder arithmetic of the AC key stage (ac_history_hash_steps:
wavefront ballots and device intrinsics) cannot be compiled for the host without changing what the existing kernels compile to; the
harness takes ACHistory::hash of a window from the oracle there, and tests/test_gpu_export_entropy.py covers that arithmetic."""
import os
import re
import shutil
import subprocess

import pytest

from weath3rb0i_amd import _lib as L
from tests import export_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "export_entropy_lanes.cpp")
ORACLE = os.path.join(ROOT, "oracle")
needs_cc = pytest.mark.skipif(shutil.which("g++") is None or shutil.which("gcc") is None, reason="gcc / g++ not found")

D_IN = "blob:0:300000"   # the blob: markov_text(300000) | lcg_text(300000) | markov_text(70000)
INIT = "ac:8:book1 11 3"   # init_model(): OrderNEntropy(11, 3, ACHistory(8, StationaryModel::for_book1()))
HUFF_D = "huff:12:12:300000"   # HuffHistory::new(D, 12, 12)
# id -> (input, history and shape, contexts met, halvings, contexts that halve): the issue's table, taken there with the oracle
ROWS = {"Z0": ("ffz:0:65600", INIT, 9, 8, 8), "Z2": ("ffz:2:65600", INIT, 20, 8, 8),
        "AC1": (D_IN, "ac:1:book1 4 3", 16, 31, 16), "H62": (D_IN, HUFF_D + " 6 2", 24, 25, 13),
        "INIT": (D_IN, INIT, 1114, 0, 0), "AC16": (D_IN, "ac:16:new 16 3", 6588, 0, 0),
        "H11": (D_IN, HUFF_D + " 11 3", 262, 0, 0), "H19": (D_IN, HUFF_D + " 19 3", 15764, 0, 0)}
EPOCHS = (1024, 4096, 5120, 65536, 0)   # 0: the length rounded up to whole KiB (one epoch)
ZRUN = "zrun:3000:5000:100:3000"   # D[:3000] + 5000 zero bytes + 100 x 0xFF + D[3000:6000]: bytes 0 and 0xFF have no code in D's table
SHORT = list(range(0, 50)) + list(range(1000, 1060))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "export_entropy", SRC, oracle=ORACLE)


def answers(harness, cases, name, exe=None):
    return H.answers(harness, cases, name, exe=exe, text=("fold", "hbytes"))


def directed_cases():
    return [("exp %s %s %d %d" % (inp, shape, e, k % 16), key, e) for k, (key, (inp, shape, _, _, _)) in enumerate(ROWS.items()) for e in EPOCHS]


@needs_cc
def test_the_table_rows_at_every_epoch_size(harness):
    cases = directed_cases()
    got = answers(harness, [c for c, _, _ in cases], "directed")
    for (case, key, e), g in zip(cases, got):
        _, _, met, halvings, contexts = ROWS[key]
        assert (g["nonzero"], g["halvings"], g["halvctx"]) == (met, halvings, contexts), (case, g)   # (the literal's, and the form's equal them)
        assert contexts <= g["replays"] <= halvings, (case, g)
        if e == 0:
            assert g["epochs"] == 1 and g["replays"] == contexts, (case, g)   # one epoch: one replay per context, however many halvings
        assert g["fixed"] == 0, (case, g)   # (no byte of D lacks a code in D's own table)
    for key in ("Z0", "Z2"):   # the hash of the empty history is 255 here, step 0 goes to context 0 all the same
        g = [x for (_, k, _), x in zip(cases, got) if k == key][0]
        assert g["e0"] != 0 and g["e2040"] != 0


@needs_cc
def test_halvings_on_the_epoch_edges_and_piece_cuts_there(harness):
    """p bytes 0xFF before the zeros under init_model(): the halvings' bytes come from the literal run; with epochs of 4,096 bytes they fall on an
    epoch's last bytes or the next one's first for some p; the stream is cut into pieces at each such byte, behind it, at both, and at (4096, it)"""
    lit = answers(harness, ["exp ffz:%d:65600 %s 4096 0" % (p, INIT) for p in range(4)], "edges_lit")
    cases = []
    for p, g in enumerate(lit):
        assert g["halvings"] == 8 and g["replays"] == 8
        for h in map(int, g["hbytes"].split(",")):
            for a in (5, 16, 17):
                cases.append("exp ffz:%d:65600 %s 4096 %d" % (p, INIT, a))
            for cuts in ((h,), (h + 1,), (h, h + 1), (4096, h)):
                cases.append("exp ffz:%d:65600 %s 4096 3 %s" % (p, INIT, " ".join(map(str, cuts))))
    assert any(int(h) % 4096 in (0, 4095) for g in lit for h in g["hbytes"].split(","))
    got = answers(harness, cases, "edges")
    assert all(g["halvings"] == 8 and g["replays"] == 8 for g in got)


@needs_cc
def test_pieces_cut_within_eight_bytes_of_each_other_and_of_the_start(harness):
    """the AC window's carry is eight bytes: pieces shorter than that, one after the other, and from the stream's first bytes on; the
    Huffman seed across the same cuts"""
    cases = []
    for shape in (INIT, "ac:16:new 16 3", "ac:24:new 12 5", HUFF_D + " 11 3", HUFF_D + " 19 3"):
        whole = "exp blob:1000:70000 %s 4096 2" % shape
        cases += [whole, "exp blob:1000:70000 %s 5120 7 1 2 3 5 8 9 15 16 17 24 1030 1033 1041 20001 20002 20009" % shape,
                  "exp blob:1000:70000 %s 0 9 7 4099 4100 4107" % shape]
    got = answers(harness, cases, "carry")
    assert [g["fold"] for g in got[0::3]] == [g["fold"] for g in got[1::3]] == [g["fold"] for g in got[2::3]]


@needs_cc
def test_huffman_keys_through_a_run_of_zero_length_codes(harness):
    cases = []
    for shape in ("11 3", "19 3"):
        for e in (1024, 4096, 0):
            cases.append("exp %s %s %s %d %d" % (ZRUN, HUFF_D, shape, e, e % 7))
            # pieces cut inside the run, at its first byte and at its last byte (bytes 3000 .. 8099 have no code)
            for cuts in ((5000,), (3000,), (8099,), (3000, 3001, 5000, 8099, 8100)):
                cases.append("exp %s %s %s %d 3 %s" % (ZRUN, HUFF_D, shape, e, " ".join(map(str, cuts))))
    got = answers(harness, cases, "zrun")
    assert all(g["len0"] == 0 and g["len255"] == 0 for g in got)   # (first of all: the run really is one of zero-length codes)
    assert all(g["fixed"] > 0 for g in got), [g["fixed"] for g in got]
    assert len({g["fold"] for g in got[:len(got) // 2]}) == 1 and len({g["fold"] for g in got[len(got) // 2:]}) == 1


def short_cases(lengths, skews):
    cases = []
    for n in lengths:
        for a in skews:
            shape = (INIT, HUFF_D + " 11 3", "ac:16:new 16 3", HUFF_D + " 19 3")[(n + a) % 4]
            cases.append("exp blob:%d:%d %s 1024 %d" % (7 * n + a, n, shape, a))
    return cases


@needs_cc
def test_short_lengths_every_skew_between_inaccessible_pages(harness):
    """lengths 0 .. 49 and 1000 .. 1059 at every pointer skew 0 .. 15 in a heap block that ends with the input, starting at a page start behind
    an inaccessible page (16) and ending at a page end before one (17).  For n >= 1 entry 0 holds step 0 and the empty history's context
    (255 << 3 under init_model()) nothing of it."""
    cases = short_cases(SHORT, list(range(18)))
    got = answers(harness, cases, "short")
    for c, g in zip(cases, got):
        n = int(c.split()[1].split(":")[2])
        assert (g["e0"] != 0) == (n >= 1), (c, g)
        if n == 1:
            assert g["e2040"] == 0 and g["nonzero"] == 8, (c, g)   # one byte: eight contexts, one per bit position, the first is context 0
    assert got[0]["epochs"] == 0 and got[0]["nonzero"] == 0   # n == 0


@needs_cc
def test_the_same_under_address_and_ub_sanitizers(harness, tmp_path):
    """A stand-alone sanitizer build of the harness (every piece and every epoch's keys live in heap blocks that end with their last byte)."""
    san = H.SAN
    why = H.sanitizer_probe(tmp_path)
    if why:
        pytest.skip(why)
    exe = str(tmp_path / "export_entropy_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + san + ["-I", ORACLE, "-o", exe, SRC, harness[3], "-lpthread", "-lm"])
    cases = [c for c, key, e in directed_cases() if key in ("Z0", "Z2", "H62") and e in (4096, 0)]
    cases += ["exp %s %s 11 3 1024 3 3000 5000 8099" % (ZRUN, HUFF_D), "exp %s %s 19 3 0 5" % (ZRUN, HUFF_D),
              "exp blob:1000:20000 %s 4096 7 1 9 4099" % INIT]
    cases += short_cases((0, 1, 2, 9, 15, 16, 17, 33, 1023, 1024, 1025, 1040), (0, 1, 7, 15))
    answers(harness, cases, "san", exe=exe)


def test_constants_and_struct_equal_the_header():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "w3hip.h"), encoding="utf-8").read()
    m = re.search(r"typedef struct w3_export_entropy_profile \{(.*?)\} w3_export_entropy_profile;", hdr, re.S)
    names = re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert names == [n for n, _ in L.ExportEntropyProfile._fields_] and C.sizeof(L.ExportEntropyProfile) == 56
    assert C.sizeof(L.ExportProfile) == 40   # (its layout does not change)
    for name in ("w3_export_entropy_device", "w3_export_entropy_staged", "w3_export_entropy_get_profile"):
        assert name in L.EXPORTS
    src = open(os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_export_entropy.h"), encoding="utf-8").read()
    assert re.search(r"#define W3_EXPK_EPOCH_MAX \(1u << 24\)", src)
