"""Table preparation on the GPU (csrc/w3_prep.h): the byte histogram against np.bincount and the stationary table against
w3.StationaryModel.new (the host loop, which tests/test_host_abi.py pins to the oracle), from tensors at every pointer offset 0 .. 15 and
from host data staged in ragged pieces; the code tables built from the device's counts against the host-built ones, byte for byte,
and one AC-over-Huffman encode with such a table; W3_E_INVALID from every new context call while a job is in flight."""
import ctypes as C

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests.synth import markov_text

pytestmark = pytest.mark.gpu
T = L.W3_STAT_TILE
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, (1 << 20) + 3]
BIG = SIZES[-1]
KINDS = ("random", "one", "two", "text")


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def text():
    return markov_text(1 << 20, seed=11)


@pytest.fixture(scope="module")
def host(text):
    """BIG + 16 bytes of every kind (a slice [off, off + n) of the device copy starts `off` bytes past hipMalloc's alignment)"""
    n = BIG + 16
    rng = np.random.default_rng(12)
    two = np.empty(n, dtype=np.uint8)
    two[0::2], two[1::2] = 0x20, 0xE5
    return {"random": rng.integers(0, 256, n, dtype=np.uint8), "one": np.full(n, 0x65, dtype=np.uint8), "two": two,
            "text": np.frombuffer((text + text[:4096])[:n], dtype=np.uint8)}


@pytest.fixture(scope="module")
def dev(host):
    import torch
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in host.items()}


def bincount(a):
    return np.bincount(a, minlength=256).astype(np.uint64)


# ---- histogram ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_histogram_device_sizes_offsets(ctx, host, dev, kind):
    for n in SIZES:
        for off in range(16):
            got = ctx.histogram_device(dev[kind][off:off + n])
            assert got.dtype == np.uint64 and got.tolist() == bincount(host[kind][off:off + n]).tolist(), (kind, n, off)


def test_histogram_device_where_every_workgroup_loops(ctx):
    import torch
    n = (1 << 26) + 5   # 16,385 turns of 4 KiB over 4,096 waves
    a = np.random.default_rng(13).integers(0, 256, n + 3, dtype=np.uint8)
    a[1000:40000000] &= 0x0F   # a skewed stretch: the counts differ a lot
    d = torch.from_numpy(a).cuda()
    assert ctx.histogram_device(d[3:]).tolist() == bincount(a[3:]).tolist()
    assert ctx.histogram_of(d[3:]).tolist() == bincount(a[3:]).tolist()


def test_histogram_staged_in_ragged_pieces(ctx, host):
    a = np.concatenate([host["text"][:300000], host["random"][:200001], host["one"][:70000]])
    want = bincount(a).tolist()
    try:
        for blocks in (1, 3, 0):   # pieces of 64 KiB, of 192 KiB (the last one ragged), one piece
            ctx.set_host_chunk_blocks(blocks)
            assert ctx.histogram(a).tolist() == want, blocks
            assert ctx.histogram(a.tobytes()[:65537]).tolist() == bincount(a[:65537]).tolist(), blocks
            assert ctx.histogram(b"").tolist() == [0] * 256
    finally:
        ctx.set_host_chunk_blocks(0)


# ---- stationary ---------------------------------------------------------------------------------------------------------------------
def station(a):
    return w3.StationaryModel.new(a.tobytes() if isinstance(a, np.ndarray) else a).table


@pytest.mark.parametrize("kind", KINDS)
def test_stationary_device_sizes_offsets(ctx, host, dev, kind):
    for n in SIZES[:-1]:
        for off in range(16):
            assert ctx.stationary_table(dev[kind][off:off + n]) == station(host[kind][off:off + n]), (kind, n, off)
    assert ctx.stationary_table(dev[kind][:0]) == [32768] * 8   # eight fresh Counters
    for off in range(KINDS.index(kind), 16, 4):   # the largest size: every offset once over the four kinds
        assert ctx.stationary_table(dev[kind][off:off + BIG]) == station(host[kind][off:off + BIG]), (kind, off)


@pytest.mark.parametrize("pol", [0, 1])
def test_stationary_prefix_family(ctx, pol):
    """k bytes 0xFF in front of 65,540 zero bytes (pol 1: the values swapped): the first halving falls on byte k + 65,534.  All inputs are
    slices of one tensor, so the pointer's offset moves with k as well."""
    import torch
    ks = list(range(0, 131)) + list(range(T - 2, T + 3)) + list(range(2 * T - 1, 2 * T + 2))
    kmax, body = 2 * T + 1, 65540
    a = np.concatenate([np.full(kmax, 0x00 if pol else 0xFF, dtype=np.uint8), np.full(body, 0xFF if pol else 0x00, dtype=np.uint8)])
    d = torch.from_numpy(a).cuda()
    for k in ks:
        got = ctx.stationary_table(d[kmax - k:])
        assert got == station(a[kmax - k:]), (pol, k)


def test_stationary_batch_edges_and_many_halvings(ctx):
    import torch
    # zeros behind 0 / 7 / 8 bytes 0xFF at a 16-byte boundary: eight halvings, the 7th in the last tile of the first batch of 64 tiles (its
    # last byte for 7) or on the first byte of the next batch's first tile (8): tests/test_table_prep_cpu.py asserts those positions
    base = torch.zeros(16 + 8 + 300000, dtype=torch.uint8)
    base[16:24] = 0xFF
    d, a = base.cuda(), base.numpy()
    for k in (0, 7, 8):
        assert ctx.stationary_table(d[24 - k:]) == station(a[24 - k:]), k
    assert ctx.stationary_table(d[24:24 + 65535]) == station(a[24:24 + 65535])   # the halving on the last byte, in a short last tile
    # skewed random data: 5 to 11 halvings per position, at different bytes; zeros, ones, zeros
    rng = np.random.default_rng(3)
    sk = np.zeros(400000, dtype=np.uint8)
    for i, pr in enumerate((0.02, 0.1, 0.3, 0.5, 0.7, 0.9, 0.97, 0.999)):
        sk |= (rng.random(len(sk)) < pr).astype(np.uint8) << (7 - i)
    runs = np.concatenate([np.zeros(70000, np.uint8), np.full(70000, 0xFF, np.uint8), np.zeros(70000, np.uint8)])
    for arr in (sk, runs):
        t = torch.from_numpy(arr).cuda()
        for off in (0, 5):
            assert ctx.stationary_table(t[off:]) == station(arr[off:])
    prof = ctx.table_prep_profile(torch.from_numpy(sk).cuda())
    assert prof["table"] == station(sk) and min(prof["halvings"]) >= 5 and prof["counts"].tolist() == bincount(sk).tolist()


def test_stationary_text_and_the_staged_form(ctx, text):
    import torch
    big = np.frombuffer(text, dtype=np.uint8)
    big = np.concatenate([np.roll(big, 977 * k) for k in range(32)])   # 2^25 bytes of text: about a thousand halvings of bit 7
    want = station(big)
    assert ctx.stationary_table(torch.from_numpy(big).cuda()) == want
    assert w3.StationaryModel.new_on(ctx, big).table == want           # staged, one piece
    part = big[:7 * 65536 + 33]
    try:
        for blocks in (1, 3):
            ctx.set_host_chunk_blocks(blocks)
            assert ctx.stationary_table(part) == station(part), blocks
            assert ctx.stationary_table(b"") == [32768] * 8
    finally:
        ctx.set_host_chunk_blocks(0)


# ---- the tables and an encode --------------------------------------------------------------------------------------------------------
def test_tables_from_the_device_equal_the_host_built_ones(ctx, host, dev):
    n = 300000
    for kind in ("text", "random", "one"):
        h, d = host[kind][3:3 + n], dev[kind][3:3 + n]
        for size in range(7, 16):
            try:
                want_c, want_h, code = bytes(w3.HuffCode.new(h, size).table), bytes(w3.HuffHistory.new(h, size, 9).tables), None
            except w3.W3Error as e:
                code = e.code
            for data in (h, d):
                if code is None:
                    assert bytes(w3.HuffCode.new_on(ctx, data, size).table) == want_c, (kind, size)
                    assert bytes(w3.HuffHistory.new_on(ctx, data, size, 9).tables) == want_h, (kind, size)
                else:
                    for f in (lambda: w3.HuffCode.new_on(ctx, data, size), lambda: w3.HuffHistory.new_on(ctx, data, size, 9)):
                        with pytest.raises(w3.W3Error) as e:
                            f()
                        assert e.value.code == code == L.W3_E_INVALID, (kind, size)
    with pytest.raises(w3.W3Error):
        w3.HuffCode.new(host["random"][:n], 7)   # (the limit that is too small did occur above)


def test_encode_with_the_device_built_table(ctx, host, dev):
    data = host["text"][5:5 + 200001]
    on_host, on_dev = w3.HuffCode.new(data, 12), w3.HuffCode.new_on(ctx, dev["text"][5:5 + 200001], 12)
    a, al = ctx.aoh_encode_blocks(on_host, 16, data, 65536)
    b, bl = ctx.aoh_encode_blocks(on_dev, 16, data, 65536)
    assert a.tobytes() == b.tobytes() and al.tolist() == bl.tolist()
    code, c, cl = ctx.aoh_compress(data, 12, 16, 65536)
    assert bytes(code.table) == bytes(on_host.table) and c.tobytes() == a.tobytes() and cl.tolist() == al.tolist()


def test_invalid_while_a_job_is_in_flight(ctx, host, dev):
    model = w3.Order0()
    data = host["text"][:200000]
    d_in = dev["text"][:200000]
    out_buf, lbuf = np.empty(2 * len(data) + 4096, dtype=np.uint8), np.zeros(4, dtype=np.uint32)
    counts, table, prof = np.zeros(256, dtype=np.uint64), (C.c_uint16 * 8)(), L.PrepProfile()
    cp, dp, hp = counts.ctypes.data_as(C.c_void_p), C.c_void_p(d_in.data_ptr()), data.ctypes.data_as(C.c_void_p)
    lib, h = ctx.lib, ctx.h
    job = ctx.encode_host_submit(model, data, 65536, out_buf, lbuf)
    try:
        assert lib.w3_histogram_device(h, dp, len(data), cp, None) == L.W3_E_INVALID
        assert lib.w3_histogram(h, hp, len(data), cp) == L.W3_E_INVALID
        assert lib.w3_stationary_table_device(h, dp, len(data), table, None) == L.W3_E_INVALID
        assert lib.w3_stationary_table_staged(h, hp, len(data), table) == L.W3_E_INVALID
        assert lib.w3_table_prep_profile(h, dp, len(data), 8, C.byref(prof)) == L.W3_E_INVALID
        assert lib.w3_histogram(h, hp, 0, cp) == L.W3_E_INVALID   # (also for an empty input)
    finally:
        ctx.encode_host_wait(job)
    assert ctx.histogram_device(d_in).tolist() == bincount(data).tolist()
    # the size limit of one device call, and bad arguments
    assert lib.w3_histogram_device(h, dp, 2**32 - 4096, cp, None) == L.W3_E_UNSUPPORTED
    assert lib.w3_stationary_table_device(h, dp, 2**32 - 4096, table, None) == L.W3_E_UNSUPPORTED
    assert lib.w3_histogram_device(h, None, 5, cp, None) == L.W3_E_INVALID and lib.w3_histogram_device(h, dp, 5, None, None) == L.W3_E_INVALID
    assert lib.w3_table_prep_profile(h, dp, 5, 3, C.byref(prof)) == L.W3_E_INVALID   # copies per counter: a power of two up to 16
