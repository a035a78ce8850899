"""Random access on AC-over-Huffman streams (w3_aoh_decode_ranges / w3_aoh_decode_ranges_device) and the sixteen-lanes-per-job decoder
k_aoh_decode_spec behind it, on the GPU.  The truth is the original data's slices; the lane-per-job kernel (W3_OPT_VARIANT decode_lane)
is the cross-check, and w3_timing.path tells which decoder ran.  Job counts around the row / wavefront boundary of the new kernel and
the 64-lane boundary of the old one, several batches, data on which every nibble hits one context four times, jobs that end inside a
nibble, a stream that is not one of ours, the refusals, the full decode under set_variant("aoh_decode_spec"), the container helper."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests.synth import markov_text, mixed_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORMS = [(), ("decode_lane",)]
CTX_BITS = [1, 8, 16, 19, 24, 25, 31]


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def want(data, ranges):
    return b"".join(data[o:o + n] for o, n in ranges)


def some_ranges(n, bs, seed):
    """crossing blocks, inside the short last block, ending at orig_len, zero-length, duplicate, overlapping, unsorted, random"""
    rng = np.random.default_rng(seed)
    last0 = (n - 1) // bs * bs
    rs = [(bs - 5, 17), (last0 + (n - last0) // 3, (n - last0) // 3), (n - 9, 9), (n // 2, 0), (0, 1), (bs - 5, 17),
          (bs // 2, 2 * bs), (3, bs + 1), (n, 0)]
    for _ in range(6):
        o = int(rng.integers(0, n))
        rs.append((o, int(rng.integers(0, min(n - o, 3 * bs) + 1))))
    return [(min(o, n), min(k, n - min(o, n))) for o, k in rs]


def blocks_of(ranges, bs):
    s = set()
    for o, n in ranges:
        if n:
            s.update(range(o // bs, (o + n - 1) // bs + 1))
    return s


def garble(comp, lens, keep, seed=5):
    """the streams of every block not in `keep` overwritten with random bytes"""
    g = np.array(comp, dtype=np.uint8, copy=True)
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    rng = np.random.default_rng(seed)
    for b in range(len(lens)):
        if b not in keep:
            g[offs[b]:offs[b + 1]] = rng.integers(0, 256, int(lens[b]), dtype=np.uint8)
    return g


def expect_path(ctx, cb, form):
    return L.W3_PATH_SPEC if (ctx.aoh_decode_spec_covers(cb) and "decode_lane" not in form) else L.W3_PATH_GENERIC


def check_host(ctx, code, cb, data, comp, lens, bs, ranges, form=()):
    """the host variant reads only the selected streams: every other one is garbage"""
    g = garble(comp, lens, blocks_of(ranges, bs))
    got = ctx.aoh_decode_ranges(code, cb, g, lens, bs, len(data), ranges)
    assert got.tobytes() == want(data, ranges), (cb, form)
    assert ctx.timing()["path"] == expect_path(ctx, cb, form), (cb, form)


def check_device(ctx, code, cb, data, comp, lens, bs, ranges, form=()):
    import torch
    w = want(data, ranges)
    d_comp = torch.from_numpy(np.ascontiguousarray(comp)).cuda()
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    d_out = torch.full((len(w) + 7,), 0xEE, dtype=torch.uint8, device="cuda")
    assert ctx.aoh_decode_ranges_device(code, cb, d_comp, d_lens, bs, len(data), ranges, d_out) == len(w)
    out = d_out.cpu().numpy()
    assert out[:len(w)].tobytes() == w and (out[len(w):] == 0xEE).all(), (cb, form)   # the bytes behind out_len are untouched
    assert ctx.timing()["path"] == expect_path(ctx, cb, form), (cb, form)


def check_forms(ctx, code, cb, data, comp, lens, bs, ranges, device=True):
    for form in FORMS:
        ctx.set_variant(*form)
        try:
            check_host(ctx, code, cb, data, comp, lens, bs, ranges, form)
            if device:
                check_device(ctx, code, cb, data, comp, lens, bs, ranges, form)
        finally:
            ctx.set_variant()


_corpus = {}


def corpus(kind, n):
    if (kind, n) not in _corpus:
        _corpus[(kind, n)] = markov_text(n, seed=17) if kind == "text" else mixed_bytes(n, seed=19)
    return _corpus[(kind, n)]


SHAPES = [(4096, 30001), (777, 12000), (65536, 2 * 65536 + 12345)]
TABLES = [("text", 9), ("text", 13), ("mixed", 9)]


def test_coverage_rule(ctx):
    assert [ctx.lib.w3_aoh_decode_spec_covers(cb) for cb in range(1, 32)] == [1] * 24 + [0] * 7


@pytest.mark.parametrize("cb", CTX_BITS)
@pytest.mark.parametrize("kind,hsize", TABLES, ids=["%s%d" % t for t in TABLES])
@pytest.mark.parametrize("bs,n", SHAPES, ids=["%d-%d" % s for s in SHAPES])
def test_ranges_every_shape_table_ctx_bits_and_form(ctx, bs, n, kind, hsize, cb):
    data = corpus(kind, n)
    code = w3.HuffCode.new(data, hsize)
    comp, lens = ctx.aoh_encode_blocks(code, cb, data, bs)
    check_forms(ctx, code, cb, data, comp, lens, bs, some_ranges(n, bs, seed=bs + n + cb))


@pytest.mark.parametrize("batch", [0, 4], ids=["one_batch", "batches_of_4"])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 65])
def test_job_counts(ctx, k, batch):
    """k distinct blocks = k jobs: a row, a wavefront less one, a wavefront, one more, and past the lane kernel's 64 lanes; again in
    batches of four jobs (W3_OPT_AOH_BATCH_BLOCKS)"""
    bs, n = 500, 70 * 500 + 123
    data = corpus("text", n)
    code = w3.HuffCode.new(data, 9)
    rng = np.random.default_rng(k)
    blocks = sorted(rng.choice(71, size=k, replace=False).tolist())
    ranges = [(b * bs + int(rng.integers(0, 50)), int(rng.integers(1, 70))) for b in blocks]
    assert len(blocks_of(ranges, bs)) == k
    ctx.set_aoh_batch_blocks(batch)
    try:
        for cb in (16, 25):
            comp, lens = ctx.aoh_encode_blocks(code, cb, data, bs)
            check_forms(ctx, code, cb, data, comp, lens, bs, ranges)
    finally:
        ctx.set_aoh_batch_blocks(0)


@pytest.mark.parametrize("cb", [1, 8])
def test_one_context_four_times_per_nibble(ctx, cb):
    """300,000 equal bytes and one other: the two-symbol table, an all-zero bit string — every nibble's four steps share one context,
    which passes 65,535 hits.  (0, 1) is a job that ends inside its first nibble."""
    data = b"a" * 300000 + b"b"
    bs = 1 << 19
    code = w3.HuffCode.new(data, 12)
    comp, lens = ctx.aoh_encode_blocks(code, cb, data, bs)
    for ranges in ([(0, 1)], [(299990, 11)], [(0, 1), (299990, 11), (0, len(data))]):
        check_forms(ctx, code, cb, data, comp, lens, bs, ranges, device=len(ranges) == 3)


@pytest.mark.parametrize("cb", [8, 24, 25])
def test_whole_input_equals_the_full_decode(ctx, cb):
    bs, n = 4096, 30001
    data = corpus("text", n)
    code = w3.HuffCode.new(data, 9)
    comp, lens = ctx.aoh_encode_blocks(code, cb, data, bs)
    whole = ctx.aoh_decode_blocks(code, cb, comp, lens, bs, n).tobytes()
    assert whole == data and ctx.timing()["path"] == L.W3_PATH_GENERIC
    for form in FORMS:
        ctx.set_variant(*form)
        try:
            assert ctx.aoh_decode_ranges(code, cb, comp, lens, bs, n, [(0, n)]).tobytes() == whole, form
        finally:
            ctx.set_variant()


@pytest.mark.parametrize("cb", [1, 8, 16, 19, 24, 31])
@pytest.mark.parametrize("bs", [4096, 65536])
def test_full_decode_with_the_sixteen_lane_decoder(ctx, bs, cb):
    """set_variant("aoh_decode_spec"): w3_aoh_decode_blocks[_device] on k_aoh_decode_spec equals the default full decode; without the
    variant the full decode stays on the lane kernel"""
    import torch
    text = corpus("text", 140001)
    code = w3.HuffCode.new(text, 9)
    for n in (0, 1, 4096, 4097, 140001):
        data = text[:n]
        comp, lens = ctx.aoh_encode_blocks(code, cb, data, bs)
        base = ctx.aoh_decode_blocks(code, cb, comp, lens, bs, n).tobytes()
        assert base == data
        if n:
            assert ctx.timing()["path"] == L.W3_PATH_GENERIC
        ctx.set_variant("aoh_decode_spec")
        try:
            assert ctx.aoh_decode_blocks(code, cb, comp, lens, bs, n).tobytes() == base, n
            if n:
                assert ctx.timing()["path"] == (L.W3_PATH_SPEC if cb <= 24 else L.W3_PATH_GENERIC)
            if n == 4097:
                d_comp = torch.from_numpy(np.ascontiguousarray(comp)).cuda()
                d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
                d_back = torch.zeros(n, dtype=torch.uint8, device="cuda")
                ctx.aoh_decode_blocks_device(code, cb, d_comp, d_lens, bs, n, d_back)
                assert d_back.cpu().numpy().tobytes() == base
            ctx.set_variant("aoh_decode_spec", "decode_lane")      # bit 1024 wins: the lane kernel
            assert ctx.aoh_decode_blocks(code, cb, comp, lens, bs, n).tobytes() == base
            if n:
                assert ctx.timing()["path"] == L.W3_PATH_GENERIC
        finally:
            ctx.set_variant()


@pytest.mark.parametrize("cb", [8, 24])
def test_a_foreign_stream_decodes_to_the_same_bytes_in_both_forms(ctx, cb):
    """random bytes under a valid length table: both kernels are deterministic decoders of one stream (a symbol also ends at max_len)"""
    bs, n = 4096, 30001
    code = w3.HuffCode.new(corpus("text", n), 9)
    rng = np.random.default_rng(23)
    lens = np.full(8, 3000, dtype=np.uint32)
    comp = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    ranges = [(100, 9000), (0, n), (29000, 1001), (4095, 2)]
    outs = []
    for form in FORMS:
        ctx.set_variant(*form)
        try:
            outs.append(ctx.aoh_decode_ranges(code, cb, comp, lens, bs, n, ranges).tobytes())
        finally:
            ctx.set_variant()
    full = ctx.aoh_decode_blocks(code, cb, comp, lens, bs, n).tobytes()
    assert outs[0] == outs[1] == want(full, ranges)


def _raw(ctx, code, cb, comp, lens, bs, n, ranges, cap, nblocks=None, in_len=None):
    rs = (L.Range * max(len(ranges), 1))()
    for i, (o, k) in enumerate(ranges):
        rs[i].offset, rs[i].len = o, k
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    olen = C.c_size_t(12345)
    a = np.ascontiguousarray(comp, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    rc = ctx.lib.w3_aoh_decode_ranges(ctx.h, C.byref(code.table), cb, a.ctypes.data_as(C.c_void_p), len(a) if in_len is None else in_len,
                                      lens.ctypes.data_as(C.c_void_p), len(lens) if nblocks is None else nblocks, bs, n, rs, len(ranges),
                                      out.ctypes.data_as(C.c_void_p), cap, C.byref(olen))
    return rc, olen.value, out


def _raw_dev(ctx, code, cb, comp, lens, bs, n, ranges, cap, nblocks=None, in_len=None):
    import torch
    rs = (L.Range * max(len(ranges), 1))()
    for i, (o, k) in enumerate(ranges):
        rs[i].offset, rs[i].len = o, k
    d_comp = torch.from_numpy(np.ascontiguousarray(comp, dtype=np.uint8)).cuda()
    d_lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32)).cuda()
    d_out = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
    olen = C.c_size_t(12345)
    rc = ctx.lib.w3_aoh_decode_ranges_device(ctx.h, C.byref(code.table), cb, C.c_void_p(d_comp.data_ptr()), d_comp.numel() if in_len is None else in_len,
                                             C.c_void_p(d_lens.data_ptr()), d_lens.numel() if nblocks is None else nblocks, bs, n, rs, len(ranges),
                                             C.c_void_p(d_out.data_ptr()), cap, C.byref(olen), None)
    return rc, olen.value, d_out.cpu().numpy()


@pytest.mark.parametrize("call", [_raw, _raw_dev], ids=["host", "device"])
def test_refusals(ctx, call):
    bs, n, cb = 4096, 30001, 16
    data = corpus("text", n)
    code = w3.HuffCode.new(data, 9)
    comp, lens = ctx.aoh_encode_blocks(code, cb, data, bs)
    ranges = [(100, 5000), (29_000, 1000)]
    rc, olen, out = call(ctx, code, cb, comp, lens, bs, n, ranges, 5999)            # out_cap one byte short: *out_len set, nothing written
    assert rc == L.W3_E_NOSPACE and olen == 6000 and not out.any()
    rc, olen, out = call(ctx, code, cb, comp, lens, bs, n, ranges, 6000)
    assert rc == L.W3_OK and olen == 6000 and out[:6000].tobytes() == want(data, ranges)
    for bad in ([(30_000, 2)], [(n + 1, 0)], [(2**64 - 1, 2)], [(1, 2**64 - 1)], [(0, 1), (n, 1)]):   # past the end, u64 wrap
        rc, olen, _ = call(ctx, code, cb, comp, lens, bs, n, bad, 100)
        assert rc == L.W3_E_INVALID, bad
    for nb in (len(lens) - 1, len(lens) + 1):                                  # nblocks does not match orig_len / block_size
        rc, _, _ = call(ctx, code, cb, comp, lens[:nb] if nb < len(lens) else np.concatenate([lens, [1]]), bs, n, ranges, 6000, nblocks=nb)
        assert rc == L.W3_E_INVALID, nb
    rc, _, _ = call(ctx, code, cb, comp, lens, bs, n, [(2**64 - 1, 2)], 6000, nblocks=len(lens) + 1)
    assert rc == L.W3_E_INVALID and b"nblocks" in ctx.lib.w3_last_error(ctx.h)   # the block count is checked first
    rc, _, _ = call(ctx, code, cb, comp, lens, bs, n, ranges, 6000, in_len=len(comp) - 1)   # the table claims more than the buffer holds
    assert rc == L.W3_E_FORMAT
    broken = list(code.codes)
    broken[max(range(256), key=lambda s: code.lens[s])] ^= 1
    rc, _, _ = call(ctx, w3.HuffCode.from_tables(broken, code.lens), cb, comp, lens, bs, n, ranges, 6000)   # an invalid table
    assert rc == L.W3_E_INVALID
    for bad_cb in (0, 32):
        rc, _, _ = call(ctx, code, bad_cb, comp, lens, bs, n, ranges, 6000)
        assert rc == L.W3_E_INVALID
    rc, olen, _ = call(ctx, code, cb, comp, lens, bs, n, [(5, 0), (n, 0)], 0)    # nothing to decode
    assert rc == L.W3_OK and olen == 0
    # while a job is in flight: W3_E_INVALID
    model = w3.Order0()
    out_buf, lbuf = np.empty(2 * n + 4096, dtype=np.uint8), np.zeros(len(lens), dtype=np.uint32)
    job = ctx.encode_host_submit(model, np.frombuffer(data, dtype=np.uint8), bs, out_buf, lbuf)
    try:
        rc, _, _ = call(ctx, code, cb, comp, lens, bs, n, ranges, 6000)
        assert rc == L.W3_E_INVALID
    finally:
        ctx.encode_host_wait(job)
    rc, olen, out = call(ctx, code, cb, comp, lens, bs, n, ranges, 6000)
    assert rc == L.W3_OK and out[:6000].tobytes() == want(data, ranges)
    # the workspace the ranges calls left behind does not disturb a full decode
    assert ctx.aoh_decode_blocks(code, cb, comp, lens, bs, n).tobytes() == data


def test_host_selection_split_into_several_calls(ctx):
    """W3_OPT_HOST_CHUNK_BLOCKS stands in for the 2 GiB cap of one device call"""
    bs, n, cb = 777, 12000, 16
    data = corpus("text", n)
    code = w3.HuffCode.new(data, 9)
    comp, lens = ctx.aoh_encode_blocks(code, cb, data, bs)
    ranges = [(0, n), (5_000, 3_000), (500, 0), (11_999, 1), (100, 3_333)]
    for cap in (1, 3):
        ctx.set_host_chunk_blocks(cap)
        try:
            assert ctx.aoh_decode_ranges(code, cb, comp, lens, bs, n, ranges).tobytes() == want(data, ranges), cap
        finally:
            ctx.set_host_chunk_blocks(0)


def test_container_helper(ctx, tmp_path):
    cli = os.path.join(ROOT, "tools", "w3")
    src = os.path.join(ROOT, "tools", "w3cli.cpp")
    if not os.path.exists(cli) or os.path.getmtime(cli) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", cli, src, "-L" + os.path.join(ROOT, "weath3rb0i_amd"), "-lw3hip",
                               "-Wl,-rpath,$ORIGIN/../weath3rb0i_amd", "-Wl,-rpath,/opt/rocm/lib"])

    def run(*args, **env):
        e = dict(os.environ)
        e.update(env)
        return subprocess.run([cli, *args], cwd=tmp_path, env=e, capture_output=True, text=True, timeout=300)

    data = markov_text(150000, seed=31) + mixed_bytes(40000, seed=32)
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)
    r = run("c", str(f), W3_MODEL="aoh:9,16")
    assert r.returncode == 0, r.stderr
    blob = (tmp_path / "corpus.bin").read_bytes()
    assert blob[:5] == b"w3bk\x02"
    ranges = [(0, 10), (65530, 20), (100000, 70000), (len(data) - 1, 1), (70000, 0), (0, len(data))]
    assert w3.aoh_container_ranges(ctx, blob, ranges).tobytes() == want(data, ranges)
    assert ctx.timing()["path"] == L.W3_PATH_SPEC
    with pytest.raises(w3.W3Error) as e:
        w3.aoh_container_ranges(ctx, blob, [(len(data), 1)])
    assert e.value.code == L.W3_E_INVALID
    for bad in (blob[:15], blob[:400], blob[:-1], b""):                 # truncated header / tables / streams
        with pytest.raises(w3.W3Error) as e:
            w3.aoh_container_ranges(ctx, bad, [(0, 1)])
        assert e.value.code == L.W3_E_FORMAT
    r = run("c", str(f))                                                 # the default model writes version 1
    assert r.returncode == 0, r.stderr
    v1 = (tmp_path / "corpus.bin").read_bytes()
    assert v1[:5] == b"w3bk\x01"
    with pytest.raises(w3.W3Error) as e:
        w3.aoh_container_ranges(ctx, v1, [(0, 1)])
    assert e.value.code == L.W3_E_FORMAT
