"""Coding from a caller's probability stream (include/w3hip.h: w3_encode_probs_device / w3_encode_stats_probs_device).
  identity   a model's own final column (export_steps_device, P_U16) fed back gives that model's streams, length table and ACStats
             counts, byte for byte — on text, and on inputs steered (tests/steer.py) into pending runs of 80, 257 and more than 65,535
             bits and into expansion, under every coder kernel with the accumulator limit that makes the fast ones hand blocks back;
  oracle     seeded random probabilities, runs of 1 and of 65535 among them, against oracle.ArithmeticCoder per bit;
  zeros      a zero anywhere is refused before any coder runs, with the step named and nothing written."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests import steer
from tests.synth import markov_text
from tests.test_gpu_parity import pair

pytestmark = pytest.mark.gpu

CODERS = ["x4", "fast", "robust", "x2", "x3", "x5"]     # W3_OPT_CODER 0 .. 5


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def _dev(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _final_column(ctx, model, d_in, bs):
    """the model's own stream, contiguous: what the coder would be given"""
    lay = ctx.steps_layout(model, "p_u16", False)
    rows = ctx.export_steps_device(model, d_in, bs, "p_u16", bit=False)
    return rows[:, lay["col_final"]].contiguous()


def _model_streams(ctx, model, data, bs):
    """(streams, length table, bit counts) of the model's own encode"""
    out, lens = ctx.encode_blocks(model, data, bs)
    return out.tobytes(), lens.tolist(), ctx.encode_stats(model, data, bs).tolist()


def _check_identity(ctx, model, data, bs):
    d_in = _dev(data)
    d_p = _final_column(ctx, model, d_in, bs)
    assert d_p.data_ptr() % 16 == 0
    want = _model_streams(ctx, model, data, bs)
    out, lens = ctx.encode_probs_device(d_in, bs, d_p)
    assert lens.cpu().tolist() == want[1]
    assert out.cpu().numpy().tobytes() == want[0]
    assert ctx.encode_stats_probs_device(d_in, bs, d_p).cpu().tolist() == want[2]


BENCH_MODEL = "o012_apm"


def _model(oracle, name):
    if name == BENCH_MODEL:
        return w3.APM(w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3)))
    return pair(oracle, name)[0]()


@pytest.mark.parametrize("name", [BENCH_MODEL, "order0"])
def test_a_models_own_stream_gives_the_models_own_output(ctx, oracle, name):
    for n, bs in [(4096 + 37, 1024), (8, 8), (3 * 65536 + 5, 65536)]:
        _check_identity(ctx, _model(oracle, name), markov_text(max(n, 64), seed=41)[:n], bs)


_RUNS = {}


def _steered(oracle, kind):
    """(data, block size) steered under Order0"""
    factory = pair(oracle, "order0")[1]
    if kind == "runs":       # pending runs of 80 and 257 bits, both first bits
        if "runs" not in _RUNS:
            _RUNS["runs"] = steer.runs(factory, [(80, 0), (80, 1), (257, 0), (257, 1)], 2, 4096)
        data, tr = _RUNS["runs"]
        assert max(tr.longest) >= 255
        return data, 4096
    data, tr = steer.counter_input("order0", factory, kind)   # hold: one run of more than 65,535 bits; anti: every block expands
    if kind == "hold":
        assert max(tr.longest) > 65535
    return data, steer.BLOCK_SIZE[kind]


@pytest.mark.parametrize("kind", ["runs", "hold", "anti"])
def test_hand_back_recode_and_raised_cap_with_a_callers_stream(oracle, kind):
    data, bs = _steered(oracle, kind)
    c = w3.Context(0)
    try:
        c.set_acc_limit(19)
        d_in = _dev(data)
        model = w3.Order0()
        d_p = _final_column(c, model, d_in, bs)
        for mode in CODERS:
            c.set_coder(mode)
            want = _model_streams(c, model, data, bs)
            out, lens = c.encode_probs_device(d_in, bs, d_p)
            if mode not in ("robust",) and kind != "anti":
                assert c.timing()["n_recoded_blocks"] >= 1, (kind, mode)      # the fast coders handed blocks back: k_coder over the caller's stream
            assert lens.cpu().tolist() == want[1], (kind, mode)
            assert out.cpu().numpy().tobytes() == want[0], (kind, mode)
            assert c.encode_stats_probs_device(d_in, bs, d_p).cpu().tolist() == want[2], (kind, mode)
        if kind == "anti":
            assert sum(want[1]) > len(data)                                    # expansion: the stripes were raised to the worst case
    finally:
        c.close()


def _random_p(n_steps, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(1, 65536, size=n_steps, dtype=np.int64)
    p[100:400] = 1
    p[700:1100] = 65535
    p[n_steps - 40:] = 1
    p[5000:5200] = rng.integers(32760, 32776, size=200)
    return p.astype(np.uint16)


def test_random_probabilities_against_the_oracles_coder(ctx, oracle):
    bs, n = 512, 3 * 512 + 5
    data = np.random.default_rng(9).integers(0, 256, size=n, dtype=np.uint8).tobytes()
    p = _random_p(8 * n, seed=10)
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8))
    streams, counts = [], []
    for o0 in range(0, n, bs):
        for sink in (oracle.ACWriter(), oracle.ACStats()):
            ac = oracle.ArithmeticCoder.new_coder()
            for t in range(8 * o0, 8 * min(o0 + bs, n)):
                ac.encode(int(bits[t]), int(p[t]), sink)
            ac.flush(sink)
            if isinstance(sink, oracle.ACStats):
                counts.append(int(sink.s.bit_count))
            else:
                streams.append(sink.bytes())
    d_in = _dev(data)
    d_p = torch.from_numpy(p.view(np.int16)).cuda()
    out, lens = ctx.encode_probs_device(d_in, bs, d_p)
    assert lens.cpu().tolist() == [len(s) for s in streams]
    assert out.cpu().numpy().tobytes() == b"".join(streams)
    assert ctx.encode_stats_probs_device(d_in, bs, d_p).cpu().tolist() == counts


@pytest.mark.parametrize("where", ["first", "last", "last_block"])
def test_a_zero_is_refused_before_any_coder_runs(ctx, oracle, where):
    bs, n = 512, 3 * 512 + 5
    data = markov_text(n, seed=3)
    d_in = _dev(data)
    p = _random_p(8 * n, seed=4)
    step = {"first": 0, "last": 8 * n - 1, "last_block": 8 * 3 * 512 + 11}[where]
    p[step] = 0
    if where == "last_block":
        p[step + 9] = 0
    d_p = torch.from_numpy(p.view(np.int16)).cuda()
    cap = int(ctx.lib.w3_max_compressed_size(n, bs))
    out = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    lens = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    total = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    rc = ctx.lib.w3_encode_probs_device(ctx.h, C.c_void_p(d_in.data_ptr()), n, bs, C.c_void_p(d_p.data_ptr()), C.c_void_p(out.data_ptr()), cap,
                                        C.c_void_p(lens.data_ptr()), C.c_void_p(total.data_ptr()), None)
    assert rc == L.W3_E_INVALID
    msg = ctx.lib.w3_last_error(ctx.h).decode()
    m = re.search(r"(\d+) zero probabilit\w+, the first at step (\d+)", msg)
    assert m and int(m.group(2)) == step and int(m.group(1)) == (2 if where == "last_block" else 1), msg
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((lens == 0x5A5A5A5A).all()) and int(total.item()) == 77
    bits = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = ctx.lib.w3_encode_stats_probs_device(ctx.h, C.c_void_p(d_in.data_ptr()), n, bs, C.c_void_p(d_p.data_ptr()), C.c_void_p(bits.data_ptr()), None)
    assert rc == L.W3_E_INVALID and bool((bits == 0x5A5A5A5A).all())
    # the context is as good as before
    model = w3.Order0()
    got, glens = ctx.encode_blocks(model, data, bs)
    want, wlens = oracle.encode_blocks(oracle.Order0(), data, bs)
    assert glens.tolist() == wlens.tolist() and got.tobytes() == want.tobytes()


def test_argument_errors(ctx):
    bs, n = 512, 1024
    d_in = _dev(markov_text(n, seed=3))
    p = torch.full((8 * n + 8,), 32768 - 65536, dtype=torch.int16, device="cuda")
    with pytest.raises(w3.W3Error) as e:
        ctx.encode_probs_device(d_in, bs, p[1:8 * n + 1])              # 2 bytes off a 16-byte boundary
    assert e.value.code == L.W3_E_INVALID and "aligned" in str(e.value)
    with pytest.raises(w3.W3Error):
        ctx.encode_probs_device(d_in, bs, p[:8 * n - 8])               # too short a stream
    with pytest.raises(w3.W3Error) as e:
        ctx.encode_probs_device(d_in[:7], bs, p[:56])                  # below the two-phase coders' minimum
    assert e.value.code == L.W3_E_UNSUPPORTED
    out, lens = ctx.encode_probs_device(d_in[:0], bs, p[:0])           # nothing to code
    assert out.numel() == 0 and lens.numel() == 0
    out, lens = ctx.encode_probs_device(d_in, bs, p[:8 * n])           # p = 1/2 everywhere: one output bit per input bit
    assert all(v >= bs for v in lens.cpu().tolist())


def test_timing_of_a_model_encode_is_untouched_and_a_callers_stream_reports_no_model_times(oracle):
    """Under W3_OPT_TIMING a two-phase encode of a model reports what it always did — path two-phase, generic_ms (the fused lane-per-block
    kernel's time) 0 — for the device call, the counting sink and the host call; coding a caller's stream reports the coder, pack and
    total times and nothing of a predict phase, whatever an earlier call on the context left in the events."""
    n, bs = 4096 + 37, 1024
    data = markov_text(n, seed=41)
    d_in = _dev(data)
    model = _model(oracle, BENCH_MODEL)
    c = w3.Context(0)
    try:
        c.set_timing(True)
        d_out = torch.empty(int(c.lib.w3_max_compressed_size(n, bs)), dtype=torch.uint8, device="cuda")
        d_lens = torch.zeros(5, dtype=torch.int32, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        c.encode_blocks_device(model, d_in, bs, d_out, d_lens, d_total)
        t = c.timing()
        assert t["path"] == L.W3_PATH_TWOPHASE and t["generic_ms"] == 0.0
        assert t["predict_ms"] > 0 and t["coder_ms"] > 0 and t["pack_ms"] > 0 and t["total_ms"] >= t["coder_ms"] and t["n_wide"] == 2
        c.encode_stats(model, data, bs)
        t = c.timing()
        assert t["path"] == L.W3_PATH_TWOPHASE and t["generic_ms"] == 0.0 and t["pack_ms"] == 0.0 and t["predict_ms"] > 0
        c.encode_blocks(model, data, bs)
        t = c.timing()
        assert t["path"] == L.W3_PATH_TWOPHASE and t["generic_ms"] == 0.0
        d_p = _final_column(c, model, d_in, bs)
        c.encode_blocks_device(model, d_in, bs, d_out, d_lens, d_total)        # leaves a predict phase's times in the job's events
        c.encode_probs_device(d_in, bs, d_p)
        t = c.timing()
        assert t["path"] == L.W3_PATH_TWOPHASE and t["coder_ms"] > 0 and t["pack_ms"] > 0 and t["total_ms"] >= t["coder_ms"]
        for k in ("predict_ms", "generic_ms", "apm_ms", "slot_ms", "achash_ms", "small_ms"):
            assert t[k] == 0.0, (k, t[k])
        assert t["n_wide"] == 0 and t["part_ms"] == [0.0] * 4 and t["rank_ms"] == [0.0] * 4 and t["n_coder_launches"] == 1
    finally:
        c.close()


def test_python_arguments_are_checked(ctx):
    d_in = _dev(markov_text(1024, seed=3))
    p = torch.full((8 * 1024,), -32768, dtype=torch.int16, device="cuda")
    for bad in (d_in.cpu(), d_in.to(torch.int8), d_in[::2]):
        with pytest.raises(w3.W3Error) as e:
            ctx.encode_probs_device(bad, 512, p)
        assert e.value.code == L.W3_E_INVALID
        with pytest.raises(w3.W3Error):
            ctx.encode_stats_probs_device(bad, 512, p)
    for fmt in ("bf16", 0, None):
        with pytest.raises(w3.W3Error) as e:
            ctx.export_steps_device(w3.Order0(), d_in, 512, fmt)
        assert e.value.code == L.W3_E_INVALID
        with pytest.raises(w3.W3Error):
            ctx.export_steps(w3.Order0(), b"x" * 64, 64, fmt)
