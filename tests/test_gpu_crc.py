"""CRC-32 per block on the GPU (w3_crc32_blocks*, w3_crc32_verify_device) and the decodes that verify it (the *_checked calls, through
the crc= keyword of the Python layer): every CRC against zlib.crc32 of the block, bit for bit; a stream with one flipped bit decodes
"successfully" to other bytes through the unchecked calls and is reported, with the block's number, by the checked ones."""
import zlib

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests.synth import markov_text, mixed_bytes

pytestmark = pytest.mark.gpu
NONE = 2**64 - 1


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def ref(data, bs):
    data = bytes(data)
    return np.array([zlib.crc32(data[o:o + bs]) for o in range(0, len(data), bs)], dtype=np.uint32)


def kinds(n, seed):
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, 256, n, dtype=np.uint8).tobytes(), "zeros": bytes(n), "ones": b"\xff" * n}


def device_crc(ctx, data, bs, offset=0):
    """crc32_blocks_device of `data` placed `offset` bytes into a tensor; checks the sentinel behind the table"""
    import torch
    n = len(data)
    nb = (n + bs - 1) // bs
    t = torch.zeros(offset + n + 3, dtype=torch.uint8)
    t[offset:offset + n] = torch.frombuffer(bytearray(data), dtype=torch.uint8) if n else t[offset:offset]
    d = t.cuda()
    d_crc = torch.full((nb + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ctx.crc32_blocks_device(d[offset:offset + n], bs, d_crc)
    out = d_crc.cpu().numpy().view(np.uint32)
    assert (out[nb:] == 0x5A5A5A5A).all(), "written past nblocks entries"
    return out[:nb]


SIZES = [1, 3, 7, 15, 16, 17, 63, 64, 65, 255, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 262144]


@pytest.mark.parametrize("bs", SIZES)
def test_crc32_blocks_device_is_zlib(ctx, bs):
    for tail in sorted({1, bs - 1} - {0}) or [0]:
        n = 3 * bs + tail
        for kind, data in kinds(n, seed=bs).items():
            got = device_crc(ctx, data, bs)
            assert got.tolist() == ref(data, bs).tolist(), (bs, tail, kind)


def test_crc32_blocks_device_large_blocks_many_blocks_and_offsets(ctx):
    for bs, n in ((1048577, 2 * 1048577 + 5), (3 * (1 << 20) + 5, 3 * (1 << 20) + 5), (1, 70001)):
        for kind, data in kinds(n, seed=n % 1000).items():
            assert device_crc(ctx, data, bs).tolist() == ref(data, bs).tolist(), (bs, n, kind)
    assert device_crc(ctx, b"", 4096).tolist() == []
    data = kinds(3 * 4097 + 100, seed=9)["random"]
    for off in (1, 3, 13):
        for bs in (17, 4097, 1025):
            assert device_crc(ctx, data, bs, offset=off).tolist() == ref(data, bs).tolist(), (off, bs)


def test_crc32_blocks_host_in_ragged_runs(ctx):
    data = kinds(7 * 4097 + 33, seed=4)["random"]
    try:
        for chunk in (0, 3):
            ctx.set_host_chunk_blocks(chunk)
            for bs in (1, 65, 4097, 65537):
                d = data[:5000] if bs == 1 else data
                assert ctx.crc32_blocks(d, bs).tolist() == ref(d, bs).tolist(), (chunk, bs)
        assert ctx.crc32_blocks(b"", 100).tolist() == []
    finally:
        ctx.set_host_chunk_blocks(0)


def test_crc32_verify_device_reports_lowest_index_and_count(ctx):
    import torch
    bs, n = 1000, 7 * 1000 + 123
    data = kinds(n, seed=11)["random"]
    d = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    good = ref(data, bs)
    nb = len(good)

    def verify(table):
        return ctx.crc32_verify_device(d, bs, torch.from_numpy(table.view(np.int32).copy()).cuda())

    assert verify(good) == (NONE, 0)
    for wrong in ({0}, {nb - 1}, {2, 5}):
        t = good.copy()
        for b in wrong:
            t[b] ^= 1
        with pytest.raises(w3.W3Error) as e:
            verify(t)
        assert e.value.code == L.W3_E_CORRUPT and e.value.bad_block == min(wrong) and e.value.n_bad == len(wrong), wrong
    assert verify(good) == (NONE, 0)


# ---- checked decodes: 4 KiB blocks, 6 blocks + a short tail
BS, N = 4096, 6 * 4096 + 1234


def corpus():
    return (markov_text(N // 2, seed=71) + mixed_bytes(N, seed=72))[:N]


def flip_in_block(comp, lens, b):
    """one bit flipped in the middle of block b's stream"""
    g = np.array(comp, dtype=np.uint8, copy=True)
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    g[int(offs[b]) + int(lens[b]) // 2] ^= 0x10
    return g


def differs_only_in_block(got, data, b):
    got, data = bytes(got), bytes(data)
    return got[:b * BS] == data[:b * BS] and got[(b + 1) * BS:] == data[(b + 1) * BS:] and got[b * BS:(b + 1) * BS] != data[b * BS:(b + 1) * BS]


def expect_corrupt(call, bad_block=3, n_bad=1):
    with pytest.raises(w3.W3Error) as e:
        call()
    assert e.value.code == L.W3_E_CORRUPT and e.value.bad_block == bad_block and e.value.n_bad == n_bad, (e.value.code, e.value.bad_block, e.value.n_bad)


MODELS = {
    "bench": lambda: w3.APM(w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3))),
    "main_default": lambda: w3.init_model(),
    "full_cm": lambda: w3.full_cm(),
}
RANGES_CLEAR = [(0, 100), (BS - 5, 17), (2 * BS + 7, BS - 7), (4 * BS, 2 * BS + 1234), (N - 9, 9), (5, 0)]    # none touches block 3
RANGES_ALL = RANGES_CLEAR + [(3 * BS - 2, 10), (3 * BS + 100, 2 * BS)]
RANGE_PREFIX = [(3 * BS, 16)]   # inside block 3, decoded long before the flipped bit is read


def want(data, ranges):
    return b"".join(data[o:o + n] for o, n in ranges)


def run_family(ctx, data, comp, lens, crc, decode, ranges, ranges_device):
    """the checks shared by a model and AC over Huffman; decode / ranges / ranges_device take (comp, ..., crc=...)"""
    import torch
    assert decode(comp, None).tobytes() == data and decode(comp, crc).tobytes() == data
    bad = flip_in_block(comp, lens, 3)
    got = decode(bad, None)   # the gap being closed: W3_OK and other bytes
    assert differs_only_in_block(got, data, 3)
    expect_corrupt(lambda: decode(bad, crc))
    wrong = crc.copy()
    wrong[3] ^= 0x80000000
    expect_corrupt(lambda: decode(comp, wrong))
    two = crc.copy()
    two[1] ^= 1
    two[6] ^= 1
    expect_corrupt(lambda: decode(comp, two), bad_block=1, n_bad=2)
    # ranges, host and device
    d_out = torch.zeros(N + 16, dtype=torch.uint8, device="cuda")

    def dev(c, rs, k):
        d_comp = torch.from_numpy(np.ascontiguousarray(c)).cuda()
        d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
        wrote = ranges_device(d_comp, d_lens, rs, d_out, k)
        return d_out[:wrote].cpu().numpy()

    for f in (ranges, dev):
        assert f(comp, RANGES_ALL, None).tobytes() == want(data, RANGES_ALL)
        assert f(comp, RANGES_ALL, crc).tobytes() == want(data, RANGES_ALL)
        assert f(bad, RANGES_CLEAR, crc).tobytes() == want(data, RANGES_CLEAR)          # block 3 is not touched: not seen
        assert f(bad, RANGE_PREFIX, None).tobytes() == want(data, RANGE_PREFIX)         # the requested bytes themselves decode fine ...
        expect_corrupt(lambda: f(bad, RANGE_PREFIX, crc))                                # ... but the block is not intact to its end
        expect_corrupt(lambda: f(bad, RANGES_ALL, crc))
        expect_corrupt(lambda: f(comp, RANGES_ALL, wrong))
    try:
        ctx.set_host_chunk_blocks(2)   # the host variants in several device calls
        assert decode(comp, crc).tobytes() == data
        expect_corrupt(lambda: decode(bad, crc))
        expect_corrupt(lambda: decode(comp, two), bad_block=1, n_bad=2)
        assert ranges(comp, RANGES_ALL, crc).tobytes() == want(data, RANGES_ALL)
        assert ranges(bad, RANGES_CLEAR, crc).tobytes() == want(data, RANGES_CLEAR)
        with pytest.raises(w3.W3Error) as e:
            ranges(bad, RANGES_ALL, crc)
        assert e.value.code == L.W3_E_CORRUPT and e.value.bad_block == 3 and e.value.n_bad >= 1   # (a split selection may count a block twice)
    finally:
        ctx.set_host_chunk_blocks(0)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_checked_decode_and_ranges(ctx, name):
    data = corpus()
    model = MODELS[name]()
    comp, lens = ctx.encode_blocks(model, data, BS)
    crc = ctx.crc32_blocks(data, BS)
    assert crc.tolist() == ref(data, BS).tolist()
    run_family(ctx, data, comp, lens, crc,
               lambda c, k: ctx.decode_blocks(model, c, lens, BS, N, crc=k),
               lambda c, rs, k: ctx.decode_ranges(model, c, lens, BS, N, rs, crc=k),
               lambda dc, dl, rs, do, k: ctx.decode_ranges_device(model, dc, dl, BS, N, rs, do, crc=k))


@pytest.mark.parametrize("variant", [(), ("decode_lane",)], ids=["default", "decode_lane"])
def test_checked_decode_and_ranges_ac_over_huffman(ctx, variant):
    data = corpus()
    code, comp, lens = ctx.aoh_compress(data, huffman_size=9, ctx_bits=16, block_size=BS)
    crc = ctx.crc32_blocks(data, BS)
    ctx.set_variant(*variant)
    try:
        run_family(ctx, data, comp, lens, crc,
                   lambda c, k: ctx.aoh_decode_blocks(code, 16, c, lens, BS, N, crc=k),
                   lambda c, rs, k: ctx.aoh_decode_ranges(code, 16, c, lens, BS, N, rs, crc=k),
                   lambda dc, dl, rs, do, k: ctx.aoh_decode_ranges_device(code, 16, dc, dl, BS, N, rs, do, crc=k))
    finally:
        ctx.set_variant()


def test_checked_calls_keep_the_unchecked_calls_errors(ctx):
    import ctypes as C
    data = corpus()
    model = MODELS["main_default"]()
    comp, lens = ctx.encode_blocks(model, data, BS)
    crc = ctx.crc32_blocks(data, BS)
    for f in (lambda k: ctx.decode_ranges(model, comp, lens, BS, N, [(N - 1, 2)], crc=k),           # a range past orig_len
              lambda k: ctx.decode_blocks(model, comp, lens[:-1], BS, N, crc=k)):                    # nblocks does not match
        for k in (None, crc):
            with pytest.raises(w3.W3Error) as e:
                f(k)
            assert e.value.code == L.W3_E_INVALID
    with pytest.raises(w3.W3Error) as e:                                                             # the table claims more than the buffer holds
        ctx.decode_blocks(model, comp[:-1], lens, BS, N, crc=crc)
    assert e.value.code == L.W3_E_FORMAT
    # no table: W3_E_INVALID
    spec = model.spec()
    out = np.empty(N, dtype=np.uint8)
    args = (ctx.h, C.byref(spec), comp.ctypes.data_as(C.c_void_p), len(comp), lens.ctypes.data_as(C.c_void_p), len(lens), BS, N, out.ctypes.data_as(C.c_void_p))
    assert ctx.lib.w3_decode_blocks_checked(*args, None) == L.W3_E_INVALID
    assert ctx.lib.w3_decode_blocks_checked(*args, C.byref(L.Check(None, 0, 0))) == L.W3_E_INVALID
    # while a job is in flight: W3_E_INVALID, as for the unchecked calls
    out_buf, lbuf = np.empty(2 * N + 4096, dtype=np.uint8), np.zeros(len(lens), dtype=np.uint32)
    job = ctx.encode_host_submit(model, np.frombuffer(data, dtype=np.uint8), BS, out_buf, lbuf)
    try:
        for f in (lambda: ctx.decode_ranges(model, comp, lens, BS, N, RANGES_ALL, crc=crc), lambda: ctx.decode_blocks(model, comp, lens, BS, N, crc=crc),
                  lambda: ctx.crc32_blocks(data, BS)):
            with pytest.raises(w3.W3Error) as e:
                f()
            assert e.value.code == L.W3_E_INVALID
    finally:
        ctx.encode_host_wait(job)
    assert ctx.decode_blocks(model, comp, lens, BS, N, crc=crc).tobytes() == data
