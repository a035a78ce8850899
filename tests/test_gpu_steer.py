"""Coders and decoders on inputs steered into long pending-bit runs (tests/steer.py; their conditions: tests/test_steer_cpu.py), at the
default accumulator limit: every coder kernel and its hand-back to k_coder, the counting sink, every decoder, the redo inside the
waits, expansion, the CM models and AC over Huffman.  The truth is always the CPU oracle's streams and length table, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests import aoh_ref, steer
from tests.synth import markov_text
from tests.test_gpu_aoh_ranges import check_forms as aoh_check_ranges
from tests.test_gpu_cm import check as cm_check, pair as cm_pair
from tests.test_gpu_parity import check_blocks, decode_both, pair

pytestmark = pytest.mark.gpu

CODERS = ["x4", "x5", "x3", "x2", "fast", "robust"]
FAST = CODERS[:5]
KINDS = ["coverage", "kept", "ends", "hold", "mixed"]      # (anti: test_expansion)


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("aoh_ref_steer")


def counter(oracle, name, kind):
    """(data, trace, block size) of an input steered under the model `name`"""
    data, tr = steer.counter_input(name, pair(oracle, name)[1], kind)
    return data, tr, tr.block_size


def truth(tr):
    """the oracle's streams and length table, as the device entry points take them (tests/test_steer_cpu.py: the trace's streams are
    oracle.encode_blocks')"""
    return np.frombuffer(tr.stream(), dtype=np.uint8), np.array(tr.lens(), dtype=np.uint32)


_bits = {}


def truth_bits(oracle, name, kind):
    """oracle.encode_stats_bits per block"""
    if (name, kind) not in _bits:
        data, tr, bs = counter(oracle, name, kind)
        model = pair(oracle, name)[1]()
        bits = []
        for o in range(0, len(data), bs):
            model.reset()
            bits.append(oracle.encode_stats_bits(model, data[o:o + bs]))
        _bits[(name, kind)] = bits
    return _bits[(name, kind)]


# ---- a. every coder at the default accumulator limit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_every_coder_at_the_default_limit(ctx, oracle, name):
    """The run-coverage input, the input of runs that every coder keeps, the block-ends input, the all-hold block with its ragged tail
    and the mixed input through every coder kernel on the two-phase path, and through the lane-per-block kernel.  On the mixed input
    the fast coders hand back
      at least the blocks in which a step is coded with 64 or more bits pending (no 64-bit accumulator holds slot + 64 ones), and
      at most the blocks whose longest run is 39 or more: the guard of w3_coder.h (and byte_c of w3_coder4.h / w3_coder5.h) drains
      whole bytes until nb < pend + 8 (pend = slot + pending ones) and gives up iff nb > 46 still, which needs pend >= 40;
    tests/test_steer_cpu.py asserts that both bounds are 44 on this input.  On plain text nothing is handed back."""
    control = markov_text(20 * 512 + 77, seed=97)
    ctx.set_path("twophase")
    try:
        for mode in CODERS:
            ctx.set_coder(mode)
            for kind in KINDS:
                data, tr, bs = counter(oracle, name, kind)
                check_blocks(ctx, oracle, name, data, bs, "twophase")
                assert ctx.timing()["path"] == 2
                if kind == "mixed" and mode in FAST:
                    n = ctx.timing()["n_recoded_blocks"]
                    lo, hi = sum(tr.handback), sum(1 for v in tr.longest if v >= 39)
                    print("n_recoded_blocks %s %s mixed: %d (bounds %d .. %d)" % (name, mode, n, lo, hi))
                    assert lo <= n <= hi, (mode, n, lo, hi)
                if kind == "kept" and mode in FAST:      # at most 38 bits pending: the fast coder's own output
                    assert ctx.timing()["n_recoded_blocks"] == 0, mode
            if mode in FAST:
                check_blocks(ctx, oracle, name, control, 512, "twophase")
                assert ctx.timing()["n_recoded_blocks"] == 0, mode
    finally:
        ctx.set_coder("x4")
        ctx.set_path("auto")
    for kind in KINDS:
        data, tr, bs = counter(oracle, name, kind)
        check_blocks(ctx, oracle, name, data, bs, "generic")
        assert ctx.timing()["path"] == 1


# ---- b. the counting sink ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_counting_sink(ctx, oracle, name):
    """encode_stats leaves unresolved pending bits out (each fast coder with its own formula; blocks that were handed back through
    k_coder's): equal to oracle.encode_stats_bits per block.  The all-hold block has counted next to nothing when its flush comes."""
    dev, _ = pair(oracle, name)
    assert truth_bits(oracle, name, "hold")[0] < 32
    try:
        for mode in CODERS:
            ctx.set_coder(mode)
            ctx.set_path("twophase")
            for kind in KINDS:
                data, tr, bs = counter(oracle, name, kind)
                got = ctx.encode_stats(dev(), data, bs)
                assert ctx.timing()["path"] == 2
                assert got.tolist() == truth_bits(oracle, name, kind), (mode, kind)
        ctx.set_coder("x4")
        ctx.set_path("generic")
        for kind in KINDS:
            data, tr, bs = counter(oracle, name, kind)
            assert ctx.encode_stats(dev(), data, bs).tolist() == truth_bits(oracle, name, kind), kind
    finally:
        ctx.set_coder("x4")
        ctx.set_path("auto")


# ---- c. decode -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_decode_every_form(ctx, oracle, name):
    """the oracle's streams through k_decode_spec (nibble and two-bit groups, both table formats, the general kernel) and the lane decoders"""
    dev, _ = pair(oracle, name)
    for kind in KINDS + ["anti"]:
        data, tr, bs = counter(oracle, name, kind)
        out, lens = truth(tr)
        assert decode_both(ctx, dev(), out, lens, bs, len(data)).tobytes() == data, kind


@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_decode_ranges_inside_runs(ctx, oracle, name):
    """ranges that end inside a long run, at a block's last byte and in the ragged last block; default form and lane-per-block decoder"""
    dev, _ = pair(oracle, name)
    for kind in ("hold", "mixed", "coverage"):
        data, tr, bs = counter(oracle, name, kind)
        out, lens = truth(tr)
        n = len(data)
        last0 = (n - 1) // bs * bs
        ranges = [(0, 1), (bs // 3, bs // 2), (bs - 9, 9), (bs - 1, 2), (last0 + 3, (n - last0) // 2), (n - 5, 5), (7, 40), (3 * bs + 30 if n > 4 * bs else 30, 100)]
        ranges = [(min(o, n), min(k, n - min(o, n))) for o, k in ranges]
        want = b"".join(data[o:o + k] for o, k in ranges)
        for form in ((), ("decode_lane",)):
            ctx.set_variant(*form)
            try:
                assert ctx.decode_ranges(dev(), out, lens, bs, n, ranges).tobytes() == want, (kind, form)
            finally:
                ctx.set_variant()


# ---- d. in flight --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_in_flight_natural_redo(ctx, oracle, name):
    """the mixed input through w3_encode_submit / w3_encode_wait, two jobs, and through w3_encode_host_submit / w3_encode_host_wait: the
    waits re-code the blocks that the fast coder handed back at the default limit"""
    import torch
    dev, _ = pair(oracle, name)
    data, tr, bs = counter(oracle, name, "mixed")
    want, wlens = truth(tr)
    host = np.frombuffer(data, dtype=np.uint8).copy()
    n, nb = len(host), len(wlens)
    d_in = torch.from_numpy(host).cuda()
    bufs = [(torch.empty(2 * n + 64 * nb + 64, dtype=torch.uint8, device="cuda"), torch.zeros(nb, dtype=torch.int32, device="cuda"),
             torch.zeros(1, dtype=torch.int64, device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()
    jobs = [ctx.encode_submit(dev(), d_in, bs, *bufs[k]) for k in range(2)]
    for k in (1, 0):
        ctx.encode_wait(jobs[k])
        assert ctx.timing()["n_recoded_blocks"] > 0, k
        d_out, d_lens, d_total = bufs[k]
        assert d_lens.cpu().numpy().astype(np.uint32).tolist() == wlens.tolist(), k
        assert d_out[: int(d_total.item())].cpu().numpy().tobytes() == want.tobytes(), k
    outs = [(np.zeros(2 * n + 64 * nb + 64, dtype=np.uint8), np.zeros(nb, dtype=np.uint32)) for _ in range(2)]
    jobs = [ctx.encode_host_submit(dev(), host, bs, *outs[k]) for k in range(2)]
    for k in range(2):
        total = ctx.encode_host_wait(jobs[k])
        assert ctx.timing()["n_recoded_blocks"] > 0, k
        assert total == len(want) and outs[k][1].tolist() == wlens.tolist() and outs[k][0][:total].tobytes() == want.tobytes(), k


# ---- e. expansion --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_expansion(ctx, oracle, name):
    """always the less probable bit: every stream longer than its block, within w3_max_compressed_size; out_cap == total succeeds and
    total - 1 is W3_E_NOSPACE with the need reported — host buffers and device-resident"""
    import torch
    dev, _ = pair(oracle, name)
    data, tr, bs = counter(oracle, name, "anti")
    want, wlens = truth(tr)
    n, nb, total = len(data), len(wlens), len(want)
    assert all(int(wlens[k]) > min(bs, n - k * bs) for k in range(nb))
    assert total <= ctx.lib.w3_max_compressed_size(n, bs)
    for path in ("twophase", "generic"):
        check_blocks(ctx, oracle, name, data, bs, path)
    out, lens = ctx.encode_blocks(dev(), data, bs, out_cap=total)
    assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes()
    host = np.frombuffer(data, dtype=np.uint8)
    spec = dev().spec()
    small, slens, olen = np.zeros(total, dtype=np.uint8), np.zeros(nb, dtype=np.uint32), C.c_size_t()
    rc = ctx.lib.w3_encode_blocks(ctx.h, C.byref(spec), host.ctypes.data_as(C.c_void_p), n, bs, small.ctypes.data_as(C.c_void_p), total - 1,
                                  C.byref(olen), slens.ctypes.data_as(C.c_void_p))
    assert rc == L.W3_E_NOSPACE and olen.value == total and slens.tolist() == wlens.tolist()
    d_in = torch.from_numpy(host.copy()).cuda()
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.encode_blocks_device(dev(), d_in, bs, d_out, d_lens, d_total)
    assert int(d_total.item()) == total and d_lens.cpu().numpy().astype(np.uint32).tolist() == wlens.tolist()
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(w3.W3Error) as e:
        ctx.encode_blocks_device(dev(), d_in, bs, d_out[: total - 1], d_lens, d_total)
    assert e.value.code == L.W3_E_NOSPACE and int(d_total.item()) == total


# ---- f. CM models --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coverage", "kept", "ends"])
@pytest.mark.parametrize("name", steer.CM_MODELS)
def test_cm_models(ctx, oracle, name, kind):
    """two-phase path, k_slot, k_cm and every decoder (check of tests/test_gpu_cm.py) on inputs steered under the CM model itself"""
    data, tr = steer.cm_input(name, cm_pair(oracle, name)[1], kind)
    cm_check(ctx, oracle, name, data, tr.block_size)


# ---- g. AC over Huffman --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["runs", "hold"])
@pytest.mark.parametrize("cb", steer.AOH_CTX_BITS)
def test_aoh(ctx, oracle, build_dir, cb, kind):
    """streams, length table and ACStats counts on both encode paths against tests/aoh_ref; the full decode (lane per block, and the
    sixteen-lane decoder where it covers) and ranges that end inside a run, in both forms of tests/test_gpu_aoh_ranges.py"""
    data, tr = steer.aoh_input(cb, kind)
    bs, n = tr.block_size, len(data)
    codes, lens = steer.aoh_table()
    code = w3.HuffCode.from_tables(codes, lens)
    want, wlens = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, cb, data, bs)
    wbits = aoh_ref.stats_bits(oracle, build_dir, codes, lens, cb, data, bs)
    assert want == tr.stream() and wlens.tolist() == tr.lens()
    for path in ("generic", "twophase"):
        ctx.set_path(path)
        try:
            out, blens = ctx.aoh_encode_blocks(code, cb, data, bs)
            assert ctx.timing()["path"] == {"generic": L.W3_PATH_GENERIC, "twophase": L.W3_PATH_TWOPHASE}[path]
            bits = ctx.aoh_encode_stats(code, cb, data, bs)
        finally:
            ctx.set_path("auto")
        assert blens.tolist() == wlens.tolist() and out.tobytes() == want, path
        assert bits.tolist() == wbits.tolist(), path
    comp = np.frombuffer(want, dtype=np.uint8)
    assert ctx.aoh_decode_blocks(code, cb, comp, wlens, bs, n).tobytes() == data
    ctx.set_variant("aoh_decode_spec")
    try:
        assert ctx.aoh_decode_blocks(code, cb, comp, wlens, bs, n).tobytes() == data
    finally:
        ctx.set_variant()
    ranges = [(0, 1), (bs // 3, bs // 2), (bs - 9, 9), (bs - 1, 2), (bs + 3, (n - bs) // 2), (n - 5, 5), (7, 40)]
    aoh_check_ranges(ctx, code, cb, data, comp, wlens, bs, ranges)
