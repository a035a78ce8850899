"""The two-phase form of AC over Huffman (W3_PATH_TWOPHASE: k_aoh_pack -> k_aoh_predict -> k_aoh_coder, weath3rb0i_amd/csrc/w3_aoh.h)
against the CPU truth of tests/aoh_ref.py and against the fused kernel (W3_PATH_GENERIC), byte for byte: streams, length tables,
ACStats bit counts, decode; rounds in which every lane meets one Counter; empty and short blocks; batches; W3_E_NOSPACE; W3_PATH_AUTO."""
import ctypes as C

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests import aoh_ref
from tests.synth import markov_text, mixed_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("aoh_ref2")


def skewed_mixed_bytes(n, seed):
    """mixed_bytes with 16 of its byte values (0xE0..0xEF) made rare: they occur 1, 1, 2, 3, 5, ... 987 times (Fibonacci counts, the
    deepest Huffman tree a histogram can ask for) at seeded positions among symbols that occur hundreds of times each, so that an
    unlimited Huffman code would be over 20 bits deep and package_merge at hsize 16 has to hand out codes of all 16 bits.  All 256
    byte values still occur."""
    a = np.frombuffer(mixed_bytes(n, seed=seed), dtype=np.uint8).copy()
    a[(a >= 0xE0) & (a < 0xF0)] ^= 0x10
    fib = [1, 1]
    while len(fib) < 16:
        fib.append(fib[-1] + fib[-2])
    pos = np.random.default_rng(seed).permutation(n)[:sum(fib)]
    a[pos] = np.repeat(np.arange(0xE0, 0xF0, dtype=np.uint8), fib)
    return a.tobytes()


@pytest.fixture(scope="module")
def corpora():
    return {"markov_text": markov_text(300003, seed=5), "mixed_bytes": skewed_mixed_bytes(262144 + 77, seed=11)}


def _code(codes, lens):
    return w3.HuffCode.from_tables(codes, lens)


def _on(ctx, path, fn):
    ctx.set_path(path)
    try:
        return fn()
    finally:
        ctx.set_path("auto")


def _encode_all(ctx, path, code, cb, data, bs):
    """(streams bytes, lens list, bits list) on one path"""
    def run():
        out, lens = ctx.aoh_encode_blocks(code, cb, data, bs)
        bits = ctx.aoh_encode_stats(code, cb, data, bs)
        return out.tobytes(), lens.tolist(), bits.tolist()
    return _on(ctx, path, run)


def _check(ctx, oracle, build_dir, codes, lens, cb, data, bs):
    code = _code(codes, lens)
    want, wlens = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, cb, data, bs)
    wbits = aoh_ref.stats_bits(oracle, build_dir, codes, lens, cb, data, bs)
    two = _encode_all(ctx, "twophase", code, cb, data, bs)
    assert two[1] == wlens.tolist(), (cb, bs)
    assert two[0] == want, (cb, bs)
    assert two[2] == wbits.tolist(), (cb, bs)
    assert _encode_all(ctx, "generic", code, cb, data, bs) == two, (cb, bs)
    # decode what was written (= the CPU truth's streams, byte for byte: asserted above); the option does not reach the decoder
    got = np.frombuffer(two[0], dtype=np.uint8)
    assert _on(ctx, "twophase", lambda: ctx.aoh_decode_blocks(code, cb, got, np.array(two[1], dtype=np.uint32), bs, len(data))).tobytes() == bytes(data)
    assert ctx.aoh_decode_blocks(code, cb, np.frombuffer(want, dtype=np.uint8), wlens, bs, len(data)).tobytes() == bytes(data)


def test_path_available(ctx):
    data = markov_text(200000, seed=2)
    code = w3.HuffCode.new(data, 12)
    ctx.set_path("twophase")
    ctx.set_timing(True)
    try:
        bits = ctx.aoh_encode_stats(code, 19, data, 65536)
        tm = ctx.timing()
        assert len(bits) == 4
        assert tm["path"] == L.W3_PATH_TWOPHASE == 2 and tm["predict_ms"] > 0 and tm["coder_ms"] > 0 and tm["generic_ms"] == 0, tm
        assert tm["predict_bytes"] > 0 and tm["coder_bytes"] > 0 and tm["n_parts"] == 1, tm
        out, lens = ctx.aoh_encode_blocks(code, 19, data, 65536)
        tm = ctx.timing()
        assert len(lens) == 4 and len(out) == int(lens.sum())
        assert tm["path"] == 2 and tm["predict_ms"] > 0 and tm["coder_ms"] > 0 and tm["generic_ms"] == 0, tm
        # the fused kernel still reports itself
        ctx.set_path("generic")
        ctx.aoh_encode_stats(code, 19, data, 65536)
        tm = ctx.timing()
        assert tm["path"] == L.W3_PATH_GENERIC and tm["generic_ms"] > 0 and tm["predict_ms"] == 0 and tm["coder_ms"] == 0, tm
    finally:
        ctx.set_timing(False)
        ctx.set_path("auto")


def test_timing_of_the_device_entry_point(ctx):
    import torch
    data = markov_text(200000, seed=2)
    code = w3.HuffCode.new(data, 12)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_out = torch.zeros(2 * len(data) + 1024, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.set_path("twophase")
    ctx.set_timing(True)
    try:
        ctx.aoh_encode_blocks_device(code, 19, d_in, 65536, d_out, d_lens, d_total)
        tm = ctx.timing()
    finally:
        ctx.set_timing(False)
        ctx.set_path("auto")
    assert tm["path"] == 2 and tm["n_parts"] == 1 and tm["generic_ms"] == 0, tm
    assert tm["predict_ms"] > 0 and tm["coder_ms"] > 0 and tm["pack_ms"] > 0 and tm["total_ms"] >= tm["predict_ms"] + tm["coder_ms"], tm


# hsize 16 gives codes of up to 16 bits on the skewed mixed_bytes.  mixed_bytes holds all 256 byte values: a code of at most 6 bits
# does not exist for it (test_no_table_of_6_bits_for_256_symbols), so hsize 6 runs on the text alone.
TABLES = [("markov_text", 6), ("markov_text", 9), ("markov_text", 13), ("markov_text", 16),
          ("mixed_bytes", 9), ("mixed_bytes", 13), ("mixed_bytes", 16)]
CTX_BITS = (1, 8, 16, 19, 24, 31)


def _parity_cases():
    """Every table at every ctx_bits in blocks of 4096 (65 lanes side by side: cheap).  The fused kernel and the decoder, which each
    check runs three times, walk a block on ONE lane, about 0.5 s per 65536 bytes: in blocks of 65536 every table runs at two ctx_bits
    and in blocks of 262144 at one, dealt round robin: at 65536 every ctx_bits meets both corpora, at 262144 every ctx_bits occurs, and
    at either size every table is there and each corpus meets both kinds of Counter table (direct up to ctx_bits 19, the exact map at
    24 and 31)."""
    for i, (kind, hsize) in enumerate(TABLES):
        yield kind, hsize, 4096, CTX_BITS
        yield kind, hsize, 65536, (CTX_BITS[i % 6], CTX_BITS[(i + 3) % 6])
        yield kind, hsize, 262144, (CTX_BITS[(i + 4) % 6],)


@pytest.mark.parametrize("kind,hsize,bs,cbs", [pytest.param(*c, id="%s-%d-%d" % c[:3]) for c in _parity_cases()])
def test_parity(ctx, oracle, build_dir, corpora, kind, hsize, bs, cbs):
    data = corpora[kind]
    codes, lens = aoh_ref.code_table(oracle, data, hsize)
    assert max(lens) <= hsize
    if (kind, hsize) == ("mixed_bytes", 16):
        assert max(lens) == 16
    for cb in cbs:
        _check(ctx, oracle, build_dir, codes, lens, cb, data, bs)


def test_no_table_of_6_bits_for_256_symbols(corpora):
    assert len(set(corpora["mixed_bytes"])) == 256
    with pytest.raises(w3.W3Error) as e:
        w3.HuffCode.new(corpora["mixed_bytes"], 6)
    assert e.value.code == L.W3_E_INVALID


@pytest.mark.parametrize("cb", [1, 8, 16, 22])
def test_identity_table_equals_ordern(ctx, cb):
    """code[s] = s, len 8: the streams are encode_blocks(OrderN(ctx_bits, 0))'s"""
    data = markov_text(300000 + 17, seed=9) + mixed_bytes(100000, seed=10)
    codes, lens = aoh_ref.identity_table()
    want, wlens = ctx.encode_blocks(w3.OrderN(cb, 0), data, 65536)
    wbits = ctx.encode_stats(w3.OrderN(cb, 0), data, 65536)
    got = _encode_all(ctx, "twophase", _code(codes, lens), cb, data, 65536)
    assert got[1] == wlens.tolist() and got[0] == want.tobytes() and got[2] == wbits.tolist()


@pytest.mark.parametrize("cb", [1, 8])
def test_same_context_rounds(ctx, oracle, build_dir, cb):
    """300,000 equal bytes under the 1-bit table: ONE Counter is hit by all 64 lanes of every round and halved again and again"""
    data = b"a" * 300000 + b"b"
    codes, lens = aoh_ref.code_table(oracle, data, 12)
    assert (codes[97], lens[97], codes[98], lens[98]) == (0, 1, 1, 1)
    _check(ctx, oracle, build_dir, codes, lens, cb, data, 1 << 19)
    _check(ctx, oracle, build_dir, codes, lens, cb, data, 65536)


def test_all_zero_table_codes_zero_bits(ctx):
    data = b"q" * 70001
    zero = w3.HuffCode.new(data, 12)
    assert not any(zero.lens)

    def run():
        assert ctx.aoh_encode_stats(zero, 16, data, 65536).tolist() == [0, 0]
        with pytest.raises(w3.W3Error) as e:
            ctx.aoh_encode_blocks(zero, 16, data, 65536)
        assert e.value.code == L.W3_E_INVALID
    _on(ctx, "twophase", run)


def test_absent_symbols_in_the_middle(ctx, oracle, build_dir):
    """bytes whose len is 0: the counting sink mirrors the reference (they contribute no bits; here also a whole block of them, L_b = 0
    between coded blocks), encode refuses"""
    text = markov_text(200000, seed=4)
    codes, lens = aoh_ref.code_table(oracle, text, 9)
    assert lens[0] == 0 and lens[1] == 0
    code = _code(codes, lens)
    bs = 4096
    bad = text[:100000] + b"\x00" + text[100000:150000] + b"\x01\x00" * 4096 + text[150000:]
    want = aoh_ref.stats_bits(oracle, build_dir, codes, lens, 16, bad, bs).tolist()
    assert 0 in want[1:-1]     # (an empty block in the middle)

    def run():
        assert ctx.aoh_encode_stats(code, 16, bad, bs).tolist() == want
        with pytest.raises(w3.W3Error) as e:
            ctx.aoh_encode_blocks(code, 16, bad, bs)
        assert e.value.code == L.W3_E_INVALID
    _on(ctx, "twophase", run)
    assert _on(ctx, "generic", lambda: ctx.aoh_encode_stats(code, 16, bad, bs).tolist()) == want


@pytest.mark.parametrize("n", [0, 1, 7, 4096, 4097])
def test_edge_sizes(ctx, oracle, build_dir, n):
    text = markov_text(5000, seed=3)
    codes, lens = aoh_ref.code_table(oracle, text, 9)
    data = text[:n]
    if n == 0:
        def run():
            out, bl = ctx.aoh_encode_blocks(_code(codes, lens), 16, data, 4096)
            assert len(out) == 0 and len(bl) == 0
            assert len(ctx.aoh_encode_stats(_code(codes, lens), 16, data, 4096)) == 0
        _on(ctx, "twophase", run)
        return
    for cb in (1, 16, 31):
        _check(ctx, oracle, build_dir, codes, lens, cb, data, 4096)


def _device_encode(ctx, code, cb, d_in, bs, nb, n):
    import torch
    d_out = torch.zeros(2 * n + 1024, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_bits = torch.zeros(nb, dtype=torch.int32, device="cuda")
    ctx.aoh_encode_blocks_device(code, cb, d_in, bs, d_out, d_lens, d_total)
    ctx.aoh_encode_stats_device(code, cb, d_in, bs, d_bits)
    total = int(d_total.item())
    return d_out[:total].cpu().numpy().tobytes(), d_lens.cpu().numpy().astype(np.uint32).tolist(), d_bits.cpu().numpy().astype(np.uint32).tolist()


@pytest.mark.parametrize("cb", [12, 24])
def test_batches(ctx, oracle, build_dir, cb):
    """11 blocks with a ragged tail in batches of 3 (3 + 3 + 3 + 2): the same output as the unbatched call, host and device entry points"""
    import torch
    bs = 8192
    data = markov_text(10 * bs + 1234, seed=6)
    codes, lens = aoh_ref.code_table(oracle, data, 11)
    code = _code(codes, lens)
    want, wlens = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, cb, data, bs)
    wbits = aoh_ref.stats_bits(oracle, build_dir, codes, lens, cb, data, bs)
    assert len(wlens) == 11
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    ctx.set_path("twophase")
    try:
        whole = _encode_all(ctx, "twophase", code, cb, data, bs)
        ctx.set_path("twophase")
        whole_dev = _device_encode(ctx, code, cb, d_in, bs, 11, len(data))
        ctx.set_aoh_batch_blocks(3)
        batched = _encode_all(ctx, "twophase", code, cb, data, bs)
        ctx.set_path("twophase")
        ctx.set_timing(True)
        batched_dev = _device_encode(ctx, code, cb, d_in, bs, 11, len(data))
        tm = ctx.timing()
    finally:
        ctx.set_timing(False)
        ctx.set_aoh_batch_blocks(0)
        ctx.set_path("auto")
    assert whole == (want, wlens.tolist(), wbits.tolist())
    assert batched == whole and whole_dev == whole and batched_dev == whole
    assert tm["path"] == 2 and tm["n_coder_launches"] == 4 and tm["n_parts"] == 1, tm     # (of the last call: the counting sink, 4 batches)


def test_nospace_on_the_device_entry_point(ctx, oracle, build_dir):
    """out_cap too small: W3_E_NOSPACE, d_total = the need, nothing written past out_cap"""
    import torch
    data = markov_text(300000 + 5, seed=8)
    bs = 65536
    codes, lens = aoh_ref.code_table(oracle, data, 9)
    code = _code(codes, lens)
    want, wlens = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, 19, data, bs)
    total, nb = len(want), len(wlens)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cap = total - 1000
    d_small = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc = _on(ctx, "twophase", lambda: ctx.lib.w3_aoh_encode_blocks_device(ctx.h, C.byref(code.table), 19, C.c_void_p(d_in.data_ptr()), len(data), bs,
                                                                           C.c_void_p(d_small.data_ptr()), cap, C.c_void_p(d_lens.data_ptr()),
                                                                           C.c_void_p(d_total.data_ptr()), None))
    assert rc == L.W3_E_NOSPACE and int(d_total.item()) == total
    assert bool((d_small[cap:] == 0xA5).all())
    assert d_lens.cpu().numpy().astype(np.uint32).tolist() == wlens.tolist()


@pytest.mark.parametrize("cb,bs", [(12, 4096), (19, 65536), (24, 65536)])
def test_auto(ctx, cb, bs):
    """W3_PATH_AUTO's output is that of both explicit paths, and timing.path names the form it took"""
    data = markov_text(400000 + 3, seed=12)
    code = w3.HuffCode.new(data, 12)
    auto = _encode_all(ctx, "auto", code, cb, data, bs)
    assert ctx.timing()["path"] in (L.W3_PATH_GENERIC, L.W3_PATH_TWOPHASE)
    assert _encode_all(ctx, "generic", code, cb, data, bs) == auto
    assert _encode_all(ctx, "twophase", code, cb, data, bs) == auto


def test_decode_and_sweep_ignore_the_option(ctx):
    data = markov_text(100000, seed=13)
    code = w3.HuffCode.new(data, 10)
    rows = ctx.sweep_ac_over_huffman(data, 16384, [code], [(0, 12), (0, 20)])
    two = _on(ctx, "twophase", lambda: ctx.sweep_ac_over_huffman(data, 16384, [code], [(0, 12), (0, 20)]))
    assert (rows == two).all()
    assert _on(ctx, "twophase", lambda: ctx.aoh_encode_stats(code, 20, data, 16384)).tolist() == rows[1].tolist()
