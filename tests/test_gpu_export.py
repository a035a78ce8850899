"""The parallel context statistics export on the GPU (csrc/w3_export.h: w3_export_counters_device / _staged) against a literal restatement
of ordern.rs:26-44 and counter.rs:20-26 — the one in tests/host/export_lanes.cpp (its `lit` case; compiled once per module) for the
directed inputs, the Python one below for the short ones — and against the unchanged one-lane Context.export_counters.  Neither yardstick
calls the code under test.  Every test here needs the new entry points: on the parent commit, where the library does not export them,
each one fails."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests.synth import lcg_text, markov_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "export_lanes.cpp")
EPOCHS = (0, 1024, 4096, 5120)   # 0: the default, one epoch for these inputs
# id -> (input of the harness, bits, align, halvings): inputs A - F of tests/test_export_cpu.py
INPUTS = {"A": ("ffz:0:20000", 4, 0, 3), "B0": ("ffz:0:65600", 3, 3, 8), "B1": ("ffz:1:65600", 3, 3, 8), "B2": ("ffz:2:65600", 3, 3, 8),
          "B3": ("ffz:3:65600", 3, 3, 8), "C": ("ffz:0:140000", 3, 3, 24), "D": ("blob:0:300000", 6, 2, 11), "E": ("blob:300000:300000", 5, 0, 1),
          "F": ("blob:600000:70000", 11, 3, 0)}
EXTRA = {"D24": ("blob:0:300000", 24, 3), "F28": ("blob:600000:70000", 28, 3), "D12": ("blob:0:300000", 12, 5)}
SHORT = (0, 1, 15, 16, 17, 1023, 1024, 1025)


def literal_run(data, bits, align):
    """OrderN::adapt + update per step, Counter::update per adapt.  -> ({ctx: n0 | n1 << 16}, [(ctx, byte) of every halving])"""
    stats, where = {}, []
    ctx = history = alignment = 0
    mask, alignment_mask = (1 << (bits - align)) - 1, (1 << align) - 1
    for k, byte in enumerate(data):
        for j in range(7, -1, -1):
            bit = (byte >> j) & 1
            c = stats.setdefault(ctx, [0, 0])
            c[bit] += 1
            if c[bit] == 0xFFFF:
                c[0], c[1] = (c[0] >> 1) + (c[0] & 1), (c[1] >> 1) + (c[1] & 1)
                where.append((ctx, k))
            history = ((history << 1) | bit) & mask
            alignment = (alignment + 1) & alignment_mask
            ctx = (history << align) | alignment
    return {c: v[0] | (v[1] << 16) for c, v in stats.items()}, where


def pairs_of(where, epoch):
    """the (context, epoch) pairs in which the literal replay halves"""
    return len({(c, k // epoch if epoch else 0) for c, k in where})


def literal(data, bits, align, epoch=None):
    """-> (table, halvings, (context, epoch) pairs that halve)"""
    t, where = literal_run(data, bits, align)
    return t, len(where), pairs_of(where, epoch)


def make_input(blob, spec):
    kind, a, b = spec.split(":")
    return blob[int(a):int(a) + int(b)] if kind == "blob" else b"\xff" * int(a) + bytes(int(b))


@pytest.fixture(scope="module")
def blob():
    return markov_text(300000) + lcg_text(300000) + markov_text(70000)


@pytest.fixture(scope="module")
def ref(tmp_path_factory, blob):
    """(key, epoch) -> (ctx: np.uint32[], value: np.uint32[], halvings, replays) of the literal replay, all computed once"""
    want = [(k, e) for k in INPUTS for e in EPOCHS] + [(k, 0) for k in EXTRA]
    shape = {k: v[:3] for k, v in list(INPUTS.items()) + list(EXTRA.items())}
    out = {}
    if shutil.which("g++") is None:   # the Python replay, once per input and shape (slow: some 15 M steps)
        runs = {}
        for k, e in want:
            if k not in runs:
                inp, bits, align = shape[k]
                t, where = literal_run(make_input(blob, inp), bits, align)
                keys = np.array(sorted(t), dtype=np.uint32)
                runs[k] = (keys, np.array([t[int(c)] for c in keys], dtype=np.uint32), where)
            out[k, e] = runs[k][:2] + (len(runs[k][2]), pairs_of(runs[k][2], e))
        return out
    d = tmp_path_factory.mktemp("export_ref")
    (d / "blob").write_bytes(blob)
    exe = str(d / "export_lanes")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, SRC])
    cases = ["lit %s %d %d %d %s" % (shape[k] + (e, d / ("%s_%d.bin" % (k, e)))) for k, e in want]
    (d / "cases").write_text("\n".join(cases) + "\n")
    lines = subprocess.run([exe, str(d / "blob"), str(d / "cases")], capture_output=True, text=True, check=True, timeout=600).stdout.splitlines()
    assert len(lines) == len(want) and all(ln.startswith("ok") for ln in lines), lines
    for (k, e), ln in zip(want, lines):
        f = dict(x.split("=") for x in ln.split()[1:])
        pairs = np.fromfile(str(d / ("%s_%d.bin" % (k, e))), dtype=np.uint32).reshape(-1, 2)
        out[k, e] = (pairs[:, 0].copy(), pairs[:, 1].copy(), int(f["halvings"]), int(f["replays"]))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.set_export_epoch(0)
    c.close()


def dense(r, bits):
    t = np.zeros(1 << bits, dtype=np.uint32)
    t[r[0]] = r[1]
    return t


def dev(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def table(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("key", list(INPUTS))
def test_device_call_equals_the_literal_replay(ctx, blob, ref, key):
    import torch
    inp, bits, align, halvings = INPUTS[key]
    d_in = dev(make_input(blob, inp))
    for e in EPOCHS:
        ctx.set_export_epoch(e)
        got = ctx.export_counters_device(w3.OrderN(bits, align), d_in)
        r = ref[key, e]
        assert r[2] == halvings   # (what the input is meant to reach)
        assert got.dtype == torch.int32 and got.numel() == 1 << bits and got.is_cuda
        assert table(got).tolist() == dense(r, bits).tolist(), (key, e)
        p = ctx.export_profile()
        assert (p["halvings"], p["replays"]) == (r[2], r[3]), (key, e, p)
        assert p["epochs"] == ((len(d_in) + e - 1) // e if e else 1), (key, e, p)   # (the default epoch is far above these lengths)
        if key == "F":
            assert p["replays"] == 0
    ctx.set_export_epoch(0)


def test_device_call_equals_the_one_lane_export(ctx, blob):
    data = blob[:20000]
    d_in = dev(data)
    for bits, align in ((11, 3), (19, 3), (4, 0), (12, 5), (16, 0)):
        n0, n1 = ctx.export_counters(w3.OrderN(bits, align), data)
        got = table(ctx.export_counters_device(w3.OrderN(bits, align), d_in))
        assert (got & 0xFFFF).tolist() == n0.tolist() and (got >> 16).tolist() == n1.tolist(), (bits, align)
    n0, n1 = ctx.export_counters(w3.Order0(), data)
    got = table(ctx.export_counters_device(w3.Order0(), d_in))
    assert (got & 0xFFFF).tolist() == n0.tolist() and (got >> 16).tolist() == n1.tolist()


def test_tensor_offsets_and_short_lengths(ctx, blob):
    base = dev(blob[:1100])
    for off in (0, 1, 7, 15):
        for n in SHORT:
            for bits, align in ((11, 3), (12, 5), (19, 3)):
                want, _, _ = literal(blob[off:off + n], bits, align)
                got = table(ctx.export_counters_device(w3.OrderN(bits, align), base[off:off + n]))
                nz = np.flatnonzero(got)
                assert nz.tolist() == sorted(want) and got[nz].tolist() == [want[c] for c in sorted(want)], (off, n, bits, align)
    assert ctx.export_profile()["replays"] == 0


def test_order_24_on_input_d_in_full(ctx, blob, ref):
    got = table(ctx.export_counters_device(w3.OrderN(24, 3), dev(blob[:300000])))
    assert np.array_equal(got, dense(ref["D24", 0], 24))


def test_order_28_on_input_f_compared_on_the_device(ctx, blob, ref):
    import torch
    keys, vals = ref["F28", 0][:2]
    got = ctx.export_counters_device(w3.OrderN(28, 3), dev(blob[600000:670000]))
    assert got.numel() == 1 << 28
    nz = torch.nonzero(got).flatten()
    assert nz.numel() == len(keys) > 1000
    assert torch.equal(nz.cpu(), torch.from_numpy(keys.astype(np.int64)))
    assert torch.equal(got[nz].cpu(), torch.from_numpy(vals.view(np.int32)))


def test_staged_in_pieces(ctx, blob, ref):
    data = blob[:300000]
    try:
        for key, bits, align in (("D", 6, 2), ("D12", 12, 5)):
            want = dense(ref[key, 0], bits)
            for blocks, pieces in ((2, 3), (1, 5), (4, 2), (0, 1)):   # three pieces; every 64 KiB block a piece; one cut; one piece
                assert not blocks or (len(data) + blocks * 65536 - 1) // (blocks * 65536) == pieces
                ctx.set_host_chunk_blocks(blocks)
                n0, n1 = ctx.export_counters_staged(w3.OrderN(bits, align), data)
                assert n0.dtype == n1.dtype == np.uint16
                assert (n0.astype(np.uint32) | (n1.astype(np.uint32) << 16)).tolist() == want.tolist(), (key, blocks)
                if key == "D":
                    assert ctx.export_profile()["halvings"] == 11
        ctx.set_host_chunk_blocks(1)
        n0, n1 = ctx.export_counters_staged(w3.OrderN(12, 5), b"")
        assert not n0.any() and not n1.any() and len(n0) == 4096
    finally:
        ctx.set_host_chunk_blocks(0)


def test_refusals(ctx, blob):
    import torch
    d_in = dev(blob[:5000])

    def code(fn):
        with pytest.raises(w3.W3Error) as e:
            fn()
        return e.value

    for model in (w3.init_model(), w3.FrozenModel(w3.Order0()), w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(29, 3)):
        e = code(lambda: ctx.export_counters_device(model, d_in))
        assert e.code == L.W3_E_UNSUPPORTED, model
        assert code(lambda: ctx.export_counters_staged(model, blob[:5000])).code == L.W3_E_UNSUPPORTED, model
    assert "w3_export_counters" in str(code(lambda: ctx.export_counters_device(w3.init_model(), d_in)))
    assert code(lambda: ctx.set_export_epoch(1000)).code == L.W3_E_INVALID
    assert code(lambda: ctx.set_export_epoch((1 << 28) + 1024)).code == L.W3_E_INVALID
    ctx.set_export_epoch(1 << 28)
    ctx.set_export_epoch(0)
    data = np.frombuffer(blob[:200000], dtype=np.uint8)
    out_buf, lbuf = np.empty(2 * len(data) + 4096, dtype=np.uint8), np.zeros(4, dtype=np.uint32)
    t = torch.zeros(2048, dtype=torch.int32, device="cuda")
    job = ctx.encode_host_submit(w3.Order0(), data, 65536, out_buf, lbuf)
    try:
        assert code(lambda: ctx.export_counters_device(w3.Order0(), d_in, t)).code == L.W3_E_INVALID
        assert code(lambda: ctx.export_counters_staged(w3.Order0(), blob[:5000])).code == L.W3_E_INVALID
    finally:
        ctx.encode_host_wait(job)
    assert not t.any()   # (refused before anything was written)


def test_two_calls_in_a_row_and_a_garbage_output_buffer(ctx, blob, ref):
    import torch
    d_in = dev(blob[:300000])
    for bits, align, key in ((6, 2, "D"), (24, 3, "D24")):   # the LDS form and the device-add form
        want = dense(ref[key, 0], bits)
        ctx.set_export_epoch(4096 if bits == 6 else 0)
        try:
            first = table(ctx.export_counters_device(w3.OrderN(bits, align), d_in))
            buf = torch.full((1 << bits,), -1515870811, dtype=torch.int32, device="cuda")   # 0xA5A5A5A5
            second = ctx.export_counters_device(w3.OrderN(bits, align), d_in, buf)
            assert second.data_ptr() == buf.data_ptr()
            assert np.array_equal(first, want) and np.array_equal(table(second), want), key   # (D was left zeroed; every entry was written)
        finally:
            ctx.set_export_epoch(0)
