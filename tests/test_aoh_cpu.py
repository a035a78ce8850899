"""AC over Huffman (bin/ac-over-huffman/main.rs), the parts that need no device: the code table against the oracle's package_merge +
canonical, the host validation every kernel index depends on, and the CPU truth helper (tests/host/aoh_ref.c) against the per-bit
composition of the oracle's parts."""
import ctypes as C

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests import aoh_ref
from tests.synth import markov_text, mixed_bytes


@pytest.fixture(scope="module")
def lib():
    from weath3rb0i_amd import build
    build.build()
    return L.load()


def _table(lib, buf, hsize):
    t = L.HuffCode()
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    rc = lib.w3_huff_code_table(a.ctypes.data_as(C.c_void_p), len(a), hsize, C.byref(t))
    return rc, t


def test_code_table_matches_oracle(lib, oracle):
    """w3_huff_code_table == package_merge + canonical of the oracle, and the length limit really shapes the tables"""
    text = markov_text(200000, seed=3)
    seen = set()
    for hs in range(6, 17):
        rc, t = _table(lib, text, hs)
        assert rc == 0, hs
        codes, lens = aoh_ref.code_table(oracle, text, hs)
        assert list(t.code) == codes and list(t.len) == lens, hs
        assert max(lens) <= hs
        seen.add(tuple(lens))
    assert len(seen) >= 9          # 35 symbols: the lengths differ for 6..14
    mixed = mixed_bytes(200000, seed=7)
    tabs = {}
    for hs in range(8, 17):
        rc, t = _table(lib, mixed, hs)
        assert rc == 0, hs
        codes, lens = aoh_ref.code_table(oracle, mixed, hs)
        assert list(t.code) == codes and list(t.len) == lens, hs
        tabs[hs] = tuple(lens)
    assert tabs[8] == (8,) * 256 and list(_table(lib, mixed, 8)[1].code) == list(range(256))   # 256 symbols at 8: the flat code
    assert tabs[9] != tabs[8] and tabs[10] != tabs[9]


def test_code_table_errors_and_degenerate_inputs(lib):
    text, mixed = markov_text(200000, seed=3), mixed_bytes(200000, seed=7)
    assert _table(lib, b"", 12)[0] == L.W3_E_INVALID          # "No symbols provided"
    assert _table(lib, text, 33)[0] == L.W3_E_INVALID         # "Max length is too big"
    assert _table(lib, text, 5)[0] == L.W3_E_INVALID          # "Max length is too small": 35 symbols
    assert _table(lib, mixed, 7)[0] == L.W3_E_INVALID         # 256 symbols
    rc, t = _table(lib, b"z" * 1000, 12)                      # one symbol: all zero, as package_merge of one count is [0]
    assert rc == 0 and not any(t.len) and not any(t.code)
    rc, t = _table(lib, b"a" * 70000 + b"b", 12)
    assert rc == 0 and (t.code[97], t.len[97], t.code[98], t.len[98]) == (0, 1, 1, 1) and sum(t.len) == 2
    with pytest.raises(w3.W3Error):
        w3.HuffCode.new(b"", 12)
    h = w3.HuffCode.new(text, 9)
    assert h.lens == list(_table(lib, text, 9)[1].len) and h.valid()


def _valid(lib, codes, lens):
    t = L.HuffCode()
    for i in range(256):
        t.code[i], t.len[i] = codes[i], lens[i]
    return lib.w3_aoh_max_compressed_size(1000, 100, C.byref(t)) != 0


def test_table_validation(lib, oracle):
    codes, lens = aoh_ref.code_table(oracle, markov_text(200000, seed=3), 9)
    assert _valid(lib, codes, lens)
    assert lib.w3_aoh_max_compressed_size(1000, 0, C.byref(w3.HuffCode.from_tables(codes, lens).table)) == 0
    assert lib.w3_aoh_max_compressed_size(1000, 100, C.byref(w3.HuffCode.from_tables(codes, lens).table)) == 2 * max(lens) * 1000 + 8 * 10 + 8
    used = [s for s in range(256) if lens[s]]
    # a non-prefix table: one symbol takes another one's prefix
    by_len = sorted(used, key=lambda s: (lens[s], codes[s]))
    short, long_ = by_len[0], by_len[-1]
    c = list(codes)
    c[long_] = codes[short] << (lens[long_] - lens[short])
    assert not _valid(lib, c, lens)
    # len 17
    l2 = list(lens)
    l2[long_] = 17
    assert not _valid(lib, codes, l2)
    # code >= 2^len
    c = list(codes)
    c[short] = 1 << lens[short]
    assert not _valid(lib, c, lens)
    # the codes of one length are not one contiguous range: two-symbol table (0,1),(1,1) is fine, (0,1),(0,1) is not; and a table
    # whose length-2 codes are 0 and 2
    z = [0] * 256
    l3 = list(z); l3[10] = 2; l3[11] = 2; l3[12] = 1
    c3 = list(z); c3[12] = 0; c3[10] = 2; c3[11] = 3
    assert _valid(lib, c3, l3)                                # canonical: len 1 -> 0; len 2 -> 10, 11
    c3[10], c3[11] = 0, 2
    assert not _valid(lib, c3, l3)
    c3[10], c3[11] = 2, 2
    assert not _valid(lib, c3, l3)
    # Kraft sum above 1: three symbols of length 1
    l4 = list(z); l4[1] = l4[2] = l4[3] = 1
    c4 = list(z); c4[2] = 1; c4[3] = 1
    assert not _valid(lib, c4, l4)
    # a permutation among symbols of equal length is the same code up to the reference's unstable sort: accepted
    same = [s for s in used if lens[s] == lens[by_len[len(by_len) // 2]]]
    assert len(same) >= 2
    c = list(codes)
    c[same[0]], c[same[-1]] = c[same[-1]], c[same[0]]
    assert c != codes and _valid(lib, c, lens)
    # the all-zero table (one-symbol input) and the container writer's replacement for it
    assert _valid(lib, z, z)
    one = w3.HuffCode.from_tables(z, z).with_single_symbol(65)
    assert one.valid() and one.lens[65] == 1 and sum(one.lens) == 1


def test_identity_table_ties_the_composition_to_the_plain_coder(oracle):
    """canonical([8] * 256) is the identity table, and with it the composed loop IS encode_stream(OrderN(B, 0))"""
    assert oracle.canonical([8] * 256) == [(s, 8) for s in range(256)]
    data = markov_text(3000, seed=5)
    codes, lens = aoh_ref.identity_table()
    for b in (8, 16, 22):
        got, _ = aoh_ref.py_encode_block(oracle, codes, lens, b, data)
        assert got == bytes(oracle.encode_stream(oracle.OrderN(b, 0), data))


def test_c_helper_equals_the_per_bit_composition(oracle, tmp_path):
    data = markov_text(4096 + 300, seed=11)
    for hs, cb in ((6, 8), (9, 16), (13, 24)):
        codes, lens = aoh_ref.code_table(oracle, data, hs)
        want, wlens = aoh_ref.py_encode_blocks(oracle, codes, lens, cb, data, 4096)
        got, glens = aoh_ref.encode_blocks(oracle, tmp_path, codes, lens, cb, data, 4096)
        assert got == want and glens.tolist() == wlens.tolist()
        assert aoh_ref.stats_bits(oracle, tmp_path, codes, lens, cb, data, 4096).tolist() == aoh_ref.py_stats_bits(oracle, codes, lens, cb, data, 4096).tolist()
        assert aoh_ref.decode_blocks(oracle, tmp_path, codes, lens, cb, got, glens, 4096, len(data)) == data
    codes, lens = aoh_ref.code_table(oracle, data, 9)
    got, glens = aoh_ref.encode_blocks(oracle, tmp_path, codes, lens, 16, data[:1000], 4096)
    assert aoh_ref.py_decode_blocks(oracle, codes, lens, 16, got, glens, 4096, 1000) == data[:1000]


def test_halving_case_on_the_cpu_truth(oracle, tmp_path):
    """70,000 equal bytes plus one other: the two-symbol table, one Counter driven through its halving"""
    data = b"a" * 70000 + b"b"
    codes, lens = aoh_ref.code_table(oracle, data, 12)
    assert (codes[97], lens[97], codes[98], lens[98]) == (0, 1, 1, 1)
    got, glens = aoh_ref.encode_blocks(oracle, tmp_path, codes, lens, 8, data, 1 << 20)
    assert aoh_ref.decode_blocks(oracle, tmp_path, codes, lens, 8, got, glens, 1 << 20, len(data)) == data


def test_sweep_driver_lines_and_tie_rule():
    """sweep.py's ac-huff driver over a fake context: the reference's lines, a later configuration replaces an equal best"""
    from weath3rb0i_amd import sweep

    class Fake:
        def sweep_ac_over_huffman(self, data, block_size, codes, configs):
            # csize 100 for every configuration but one worse
            rows = [[800] for _ in configs]
            rows[0] = [1600]
            return np.array(rows, dtype=np.uint32)

    lines = []
    data = markov_text(200000, seed=3)   # 35 symbols: 4 and 5 are too small
    best, params, table = sweep.sweep_ac_over_huffman(Fake(), data, 65536, huffman_sizes=range(4, 8), ctx_bits=range(8, 11), out=lines.append)
    assert lines[0] == "[ac-over-huff] [hsize:  4] length limit too small for the alphabet"
    assert lines[1] == "[ac-over-huff] [hsize:  5] length limit too small for the alphabet"
    assert lines[2].startswith("[ac-over-huff] [hsize:  6, ctx:  8, align: 0] csize: 200 (ratio: 0.001), ctime: ")
    assert "-> best: 100 for [hsize: 6] when [ctx: 10, align: 0]" in lines
    assert lines[-1] == "-> gloabl best: 100 for [hsize: 7, ctx: 10, align: 0]"
    assert (best, params) == (100, (7, 10)) and table[(6, 8)] == 200 and len(table) == 6
