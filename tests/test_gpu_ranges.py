"""Random-access decode (w3_decode_ranges / w3_decode_ranges_device) on the GPU: every result against the original slices, and a
whole-input range against w3_decode_blocks — over models that take every decode kernel (k_decode_spec and its instances, k_generic_nl,
k_generic, k_cm_nl, k_cm_staged, k_cm), in the five decode forms of the parity tests, at 64 KiB and small blocks with a ragged last block.
The host variant must read only the selected blocks' streams: every other stream is overwritten with garbage first."""
import os
import subprocess

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests.synth import lcg_text, markov_text, mixed_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def _huff():
    return w3.HuffHistory.new(markov_text(40000, seed=61), 12, 12)


MODELS = {
    "order0": lambda: w3.Order0(),
    "main_default": lambda: w3.init_model(),
    "order012apm": lambda: w3.APM(w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3))),   # the bench model
    "huff_11": lambda: w3.OrderNEntropy(11, 3, _huff()),
    "frozen0": lambda: w3.FrozenModel(w3.Order0()),
    "ordern_12_0": lambda: w3.OrderN(12, 0),   # alignment below 2: the lane-per-block kernels in every form
    "ordern_9_1": lambda: w3.OrderN(9, 1),
    "five_leaves": lambda: w3.BestOfTwoModel(w3.BestOfTwoModel(w3.OrderN(12, 1), w3.Order0()),
                                             w3.BestOfTwoModel(w3.BestOfTwoModel(w3.OrderN(10, 0), w3.Order1()), w3.OrderN(9, 1))),   # k_generic
    "slot_mix": lambda: w3.BestOfTwoModel(w3.SlotModel(2, 12), w3.BestOfTwoModel(w3.Order0(), w3.SlotModel(1, 12))),
    "full_cm": lambda: w3.full_cm(),
}

# the five decode forms of tests/test_gpu_parity.py decode_both: (variant names, W3_OPT_TUNE bits)
FORMS = [((), 0), (("decode_lane",), 0), ((), 16384), ((), 262144), ((), 262144 | 524288)]


def set_form(ctx, form):
    variant, tune = form
    ctx.set_variant(*variant)
    ctx.set_tune(tune)


def reset(ctx):
    ctx.set_variant()
    ctx.set_tune(0)


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


def check_both(ctx, model, data, comp, lens, bs, ranges):
    import torch
    n = len(data)
    w = want(data, ranges)
    g = garble(comp, lens, blocks_of(ranges, bs))
    got = ctx.decode_ranges(model, g, lens, bs, n, ranges)
    assert got.tobytes() == w
    d_comp = torch.from_numpy(g).cuda()
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    d_out = torch.full((len(w) + 7,), 0xEE, dtype=torch.uint8, device="cuda")
    wrote = ctx.decode_ranges_device(model, d_comp, d_lens, bs, n, ranges, d_out)
    assert wrote == len(w)
    out = d_out.cpu().numpy()
    assert out[:len(w)].tobytes() == w and (out[len(w):] == 0xEE).all()


def corpus(n, seed):
    return (markov_text(n // 2, seed=seed) + mixed_bytes(n // 4, seed=seed + 1) + lcg_text(n, seed=seed + 2))[:n]


CASES = [   # (model, block size, bytes): 64 KiB blocks and small ones, every last block ragged
    ("order0", 65536, 3 * 65536 + 4321), ("order0", 1000, 9123),
    ("main_default", 65536, 2 * 65536 + 999), ("main_default", 4096, 30001),
    ("order012apm", 65536, 2 * 65536 + 12345), ("order012apm", 777, 12000),
    ("huff_11", 65536, 65536 + 3001), ("huff_11", 2048, 20001),
    ("frozen0", 65536, 65536 + 77), ("frozen0", 3000, 10001),
    ("ordern_12_0", 65536, 65536 + 555), ("ordern_12_0", 1500, 9001),
    ("ordern_9_1", 65536, 65536 + 555), ("ordern_9_1", 1024, 8191),
    ("five_leaves", 4096, 16385),
    ("slot_mix", 65536, 65536 + 4097), ("slot_mix", 2500, 11111),
    ("full_cm", 16384, 3 * 16384 + 100), ("full_cm", 1000, 6001),
]


@pytest.mark.parametrize("name,bs,n", CASES, ids=["%s-%d-%d" % c for c in CASES])
def test_ranges_every_model_form_and_variant(ctx, name, bs, n):
    data = corpus(n, seed=n % 97)
    model = MODELS[name]()
    comp, lens = ctx.encode_blocks(model, data, bs)
    ranges = some_ranges(n, bs, seed=bs + n)
    whole = ctx.decode_blocks(model, comp, lens, bs, n).tobytes()
    assert whole == data
    for form in FORMS:
        set_form(ctx, form)
        try:
            check_both(ctx, model, data, comp, lens, bs, ranges)
            assert ctx.decode_ranges(model, comp, lens, bs, n, [(0, n)]).tobytes() == whole, form
        finally:
            reset(ctx)
    if name == "slot_mix":   # k_cm: the slot-state decoder without LDS staging
        ctx.set_variant("decode_lane", "cm_unstaged")
        try:
            check_both(ctx, model, data, comp, lens, bs, ranges)
        finally:
            reset(ctx)


def test_ranges_host_split_into_several_calls(ctx):
    """A selection larger than one device call (W3_OPT_HOST_CHUNK_BLOCKS stands in for the 2 GiB cap): the ranges are cut into parts
    and the parts go through several calls, each writing its stretch of the output."""
    bs, n = 1000, 25_500
    data = corpus(n, seed=3)
    model = MODELS["order012apm"]()
    comp, lens = ctx.encode_blocks(model, data, bs)
    ranges = [(0, n), (12_345, 7_000), (500, 0), (24_999, 501), (100, 3_333), (0, n)]
    for cap in (1, 2, 3, 7):
        ctx.set_host_chunk_blocks(cap)
        try:
            assert ctx.decode_ranges(model, comp, lens, bs, n, ranges).tobytes() == want(data, ranges), cap
        finally:
            ctx.set_host_chunk_blocks(0)


def _raw(ctx, model, comp, lens, bs, n, ranges, cap, nblocks=None, in_len=None):
    spec = model.spec()
    import ctypes as C
    rs = (L.Range * max(len(ranges), 1))()
    for i, (o, k) in enumerate(ranges):
        rs[i].offset, rs[i].len = o, k
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    olen = C.c_size_t(12345)
    a = np.ascontiguousarray(comp, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    rc = ctx.lib.w3_decode_ranges(ctx.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a) if in_len is None else in_len,
                                  lens.ctypes.data_as(C.c_void_p), len(lens) if nblocks is None else nblocks, bs, n, rs, len(ranges),
                                  out.ctypes.data_as(C.c_void_p), cap, C.byref(olen))
    return rc, olen.value, out


def _raw_dev(ctx, model, comp, lens, bs, n, ranges, cap, nblocks=None, in_len=None):
    import ctypes as C
    import torch
    spec = model.spec()
    rs = (L.Range * max(len(ranges), 1))()
    for i, (o, k) in enumerate(ranges):
        rs[i].offset, rs[i].len = o, k
    d_comp = torch.from_numpy(np.ascontiguousarray(comp, dtype=np.uint8)).cuda()
    d_lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32)).cuda()
    d_out = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
    olen = C.c_size_t(12345)
    rc = ctx.lib.w3_decode_ranges_device(ctx.h, C.byref(spec), C.c_void_p(d_comp.data_ptr()), d_comp.numel() if in_len is None else in_len,
                                         C.c_void_p(d_lens.data_ptr()), d_lens.numel() if nblocks is None else nblocks, bs, n, rs, len(ranges),
                                         C.c_void_p(d_out.data_ptr()), cap, C.byref(olen), None)
    return rc, olen.value, d_out.cpu().numpy()


@pytest.mark.parametrize("call", [_raw, _raw_dev], ids=["host", "device"])
def test_ranges_errors_and_workspace_reuse(ctx, call):
    bs, n = 4096, 40_000
    data = corpus(n, seed=11)
    model = MODELS["order0"]()
    comp, lens = ctx.encode_blocks(model, data, bs)
    ranges = [(100, 5000), (39_000, 1000)]
    rc, olen, _ = call(ctx, model, comp, lens, bs, n, ranges, 5999)            # out_cap one byte short
    assert rc == L.W3_E_NOSPACE and olen == 6000
    rc, olen, out = call(ctx, model, comp, lens, bs, n, ranges, 6000)
    assert rc == L.W3_OK and olen == 6000 and out[:6000].tobytes() == want(data, ranges)
    for bad in ([(39_999, 2)], [(n + 1, 0)], [(2**64 - 1, 2)], [(1, 2**64 - 1)], [(0, 1), (n, 1)]):
        rc, olen, _ = call(ctx, model, comp, lens, bs, n, bad, 100)
        assert rc == L.W3_E_INVALID, bad
    for nb in (len(lens) - 1, len(lens) + 1):                                  # nblocks does not match orig_len / block_size
        rc, _, _ = call(ctx, model, comp, lens[:nb] if nb < len(lens) else np.concatenate([lens, [1]]), bs, n, ranges, 6000, nblocks=nb)
        assert rc == L.W3_E_INVALID, nb
    rc, _, _ = call(ctx, model, comp, lens, bs, n, ranges, 6000, in_len=len(comp) - 1)   # the table claims more than the buffer holds
    assert rc == L.W3_E_FORMAT
    rc, olen, _ = call(ctx, model, comp, lens, bs, n, [(5, 0), (n, 0)], 0)    # nothing to decode
    assert rc == L.W3_OK and olen == 0
    # the workspace the ranges calls left behind does not disturb a full decode
    assert ctx.decode_blocks(model, comp, lens, bs, n).tobytes() == data
    # while a job is in flight: W3_E_INVALID
    out_buf, lbuf = np.empty(2 * n + 4096, dtype=np.uint8), np.zeros(len(lens), dtype=np.uint32)
    job = ctx.encode_host_submit(model, np.frombuffer(data, dtype=np.uint8), bs, out_buf, lbuf)
    try:
        rc, _, _ = call(ctx, model, comp, lens, bs, n, ranges, 6000)
        assert rc == L.W3_E_INVALID
    finally:
        ctx.encode_host_wait(job)
    rc, olen, out = call(ctx, model, comp, lens, bs, n, ranges, 6000)
    assert rc == L.W3_OK and out[:6000].tobytes() == want(data, ranges)


def test_ranges_at_scale(ctx):
    """1e8 bytes in 64 KiB blocks, device-resident, 4,096 random ranges of up to 4 KiB (plus one long one) through both variants."""
    import torch
    from tools import synth
    n, bs = 100_000_000, 65536
    host = synth.text(n, seed=1)
    model = MODELS["order012apm"]()
    nb = (n + bs - 1) // bs
    d_in = torch.from_numpy(host).cuda()
    d_comp = torch.empty(n // 2 + 64 * nb + 1024, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.encode_blocks_device(model, d_in, bs, d_comp, d_lens, d_total)
    total = int(d_total.item())
    rng = np.random.default_rng(7)
    offs = rng.integers(0, n - 4096, 4096)
    ranges = np.stack([offs, rng.integers(0, 4097, 4096)], axis=1)
    ranges = np.concatenate([ranges, [[n - 3 * bs - 11, 3 * bs + 11]]])
    w = b"".join(host[o:o + k].tobytes() for o, k in ranges.tolist())
    d_out = torch.empty(len(w), dtype=torch.uint8, device="cuda")
    assert ctx.decode_ranges_device(model, d_comp[:total], d_lens, bs, n, ranges, d_out) == len(w)
    assert d_out.cpu().numpy().tobytes() == w
    comp, lens = d_comp[:total].cpu().numpy(), d_lens.cpu().numpy().view(np.uint32)
    assert ctx.decode_ranges(model, comp, lens, bs, n, ranges[:512]).tobytes() == w[:int(ranges[:512, 1].sum())]


@pytest.fixture(scope="module")
def cli():
    exe = os.path.join(ROOT, "tools", "w3")
    src = os.path.join(ROOT, "tools", "w3cli.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src, "-L" + os.path.join(ROOT, "weath3rb0i_amd"), "-lw3hip",
                               "-Wl,-rpath,$ORIGIN/../weath3rb0i_amd", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cli_extract(cli, tmp_path):
    data = markov_text(150000, seed=5) + mixed_bytes(60000, seed=6)
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)

    def run(*args, **env):
        e = dict(os.environ)
        e.update(env)
        return subprocess.run([cli, *args], cwd=tmp_path, env=e, capture_output=True, text=True, timeout=300)

    r = run("c", str(f), W3_MODEL="order012apm")
    assert r.returncode == 0, r.stderr
    for o, k in ((0, 10), (65530, 20), (100000, 110000), (len(data) - 1, 1), (70000, 0)):   # (65530, 20) and the long one cross blocks
        r = run("r", "corpus.bin", str(o), str(k), W3_MODEL="order012apm")
        assert r.returncode == 0, r.stderr
        assert "Extraction took" in r.stdout
        assert (tmp_path / "corpus.part").read_bytes() == data[o:o + k], (o, k)
    assert run("r", "corpus.bin", str(len(data)), "1", W3_MODEL="order012apm").returncode == 1   # past the end
    assert run("r", "corpus.bin", "-1", "1").returncode == 1
    assert run("r", "corpus.bin", "1").returncode == 1
    assert run("r", "missing.bin", "0", "1").returncode == 1
    r = run("c", str(f), W3_CONTAINER="w30i")
    assert r.returncode == 0, r.stderr
    r = run("r", "corpus.bin", "0", "10")
    assert r.returncode == 1 and "block container" in r.stderr
    assert run("x", "nothing").returncode == 1
