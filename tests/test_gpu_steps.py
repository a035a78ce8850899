"""The per-step statistics export (include/w3hip.h "per-step statistics"; csrc/w3_steps.h) against the CPU oracle: every column of
every row, for equality.  Expected rows are built column by column, block by block (blocks restart the model): leaf l = predict_all of
that leaf alone, mix = the nested tree without its APM nodes, stage j = the tree with the chain cut after stage j, bit = the unpacked
input; the STRETCH formats go through oracle.stretch and numpy."""
import ctypes as C

import numpy as np
import pytest
import torch

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests.synth import lcg_text, markov_text
from tests.test_gpu_parity import huff_pair

pytestmark = pytest.mark.gpu

BOOK1 = [1, 50188, 62497, 15819, 22545, 31499, 22988, 29616]


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def _leaf(name, oracle):
    """(device leaf, oracle leaf) of a named leaf"""
    o = oracle
    if name == "o0":
        return w3.Order0(), o.Order0()
    if name == "o1":
        return w3.Order1(), o.Order1()
    if name == "o2":
        return w3.OrderN(27, 3), o.OrderN(27, 3)
    if name == "frozen1":
        return w3.FrozenModel(w3.Order1()), o.FrozenModel(o.Order1())
    if name == "ac":
        return w3.init_model(), o.OrderNEntropy(11, 3, o.ACHistory(8, o.StationaryModel.from_table(BOOK1)))
    if name == "huff":
        dev_h, orc_t = huff_pair(o, "text")
        return w3.OrderNEntropy(11, 3, dev_h), o.OrderNEntropy(11, 3, o.HuffHistory(tables=orc_t))
    if name == "slot":
        return w3.SlotModel(2, 10), o.SlotModel(2, 10)
    if name == "wave":
        return w3.OrderN(22, 2), o.OrderN(22, 2)
    bits = int(name[1:])          # "n8": OrderN(8, 3)
    return w3.OrderN(bits, 3), o.OrderN(bits, 3)


NINE = ["o0", "n4", "n5", "n6", "n7", "n8", "n9", "n10", "o1"]
SPECS = {   # name -> (leaves, APM stages as (context kind, rate))
    "o0": (["o0"], []),
    "o0_apm": (["o0"], [(0, 7)]),                       # the single leaf's stream is where the stage writes: the in-place hazard
    "o012": (["o0", "o1", "o2"], []),
    "o012_apm": (["o0", "o1", "o2"], [(0, 7)]),
    "o012_apm2": (["o0", "o1", "o2"], [(0, 7), (1, 6)]),
    "frozen": (["o0", "frozen1", "o1"], []),
    "frozen_first_apm": (["frozen1", "o0"], [(0, 7)]),
    "five": (["o0", "n5", "n7", "o1", "n9"], []),
    "nine_apm": (NINE, [(0, 7)]),                       # more than 8 streams: twophase_apm merges them first
    "ac": (["ac"], []),
    "huff": (["huff"], []),
    "slot": (["slot"], []),
    "wave": (["wave"], []),
    "o0_apm1": (["o0"], [(1, 6)]),                      # an ORDER1 stage first: in place over the single leaf's stream too
}


def _nest(models, two):
    m = models[0]
    for nxt in models[1:]:
        m = two(m, nxt)
    return m


def device_model(oracle, name):
    leaves, apms = SPECS[name]
    m = _nest([_leaf(l, oracle)[0] for l in leaves], w3.BestOfTwoModel)
    for kind, rate in apms:
        m = w3.APM(m, kind, rate)
    return m


def _per_block(oracle, model, data, bs):
    out = []
    for o0 in range(0, len(data), bs):
        model.reset()
        out.append(oracle.predict_all(model, data[o0:o0 + bs]))
    return np.concatenate(out)


_P = {}


def expected_p(oracle, name, data, bs, key):
    """uint16 [8 n, C] with the bit column: the P_U16 rows.  Computed once per (spec, input) and shared."""
    if (name, key) not in _P:
        leaves, apms = SPECS[name]
        cols = [_per_block(oracle, _leaf(l, oracle)[1], data, bs) for l in leaves]

        def tree(n_stages):
            m = _nest([_leaf(l, oracle)[1] for l in leaves], oracle.BestOfTwoModel)
            for kind, rate in apms[:n_stages]:
                m = oracle.APM(m, kind, rate)
            return m
        for j in range(len(apms) + 1):
            cols.append(_per_block(oracle, tree(j), data, bs))
        cols.append(np.unpackbits(np.frombuffer(data, dtype=np.uint8)).astype(np.uint16))
        rows = np.stack(cols, axis=1)
        rows.setflags(write=False)
        _P[(name, key)] = rows
    return _P[(name, key)]


_STRETCH = {}


def as_format(oracle, rows_p, fmt):
    """the expected rows of a format from the P_U16 rows (bit column last)"""
    if fmt == "p_u16":
        return rows_p
    if "t" not in _STRETCH:
        _STRETCH["t"] = np.array([oracle.stretch(p) for p in range(65536)], dtype=np.int16)
    s = _STRETCH["t"][rows_p[:, :-1]]
    bit = rows_p[:, -1:]
    if fmt == "stretch_i16":
        return np.concatenate([s, bit.astype(np.int16)], axis=1)
    f = (s.astype(np.float64) / 256).astype(np.float16)
    assert (f.astype(np.float64) * 256 == s).all()
    return np.concatenate([f, bit.astype(np.float16)], axis=1)


def _np(t):
    """a row tensor as numpy, bit for bit (torch.uint16 where the build has it)"""
    if t.dtype == torch.float16:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16 if t.dtype != torch.int16 else np.int16)


def _same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.dtype == np.float16:
        got, want = got.view(np.uint16), want.view(np.uint16)
    else:
        got, want = got.view(np.uint16), want.astype(got.dtype).view(np.uint16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (row, column)", bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))


def text(n, seed=5):
    return markov_text(n, seed=seed) if n >= 64 else lcg_text(n, seed=seed)


FIVE_BLOCKS = (4096 + 37, 1024)        # 5 blocks, a short last one, n no multiple of 64
SHAPES = [(8, 8), FIVE_BLOCKS, (63, 64), (64, 64), (65, 32), (191, 64), (193, 1024)]   # (n, block size); 64 k +- 1 around one wavefront tile


@pytest.mark.parametrize("name", sorted(SPECS))
def test_p_u16_rows_of_every_spec(ctx, oracle, name):
    for n, bs in SHAPES if name in ("o0", "o0_apm", "o012_apm") else [FIVE_BLOCKS, (65, 32)]:
        data = text(n)
        d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        model = device_model(oracle, name)
        want = expected_p(oracle, name, data, bs, (n, bs))
        lay = ctx.steps_layout(model, "p_u16", True)
        assert lay["n_cols"] == want.shape[1]
        rows = ctx.export_steps_device(model, d_in, bs, "p_u16", bit=True)
        assert tuple(rows.shape) == (8 * n, lay["n_cols"]) and rows.is_cuda
        _same(_np(rows), want)
        rows = ctx.export_steps_device(model, d_in, bs, "p_u16", bit=False)      # the same without the bit column
        _same(_np(rows), want[:, :-1])
        # the last model column is what the coder is given: w3_predict_blocks
        assert _np(rows)[:, lay["col_final"]].tolist() == ctx.predict_blocks(model, data, bs).tolist()


@pytest.mark.parametrize("name", ["o0_apm", "o012_apm2", "frozen", "nine_apm"])
@pytest.mark.parametrize("fmt", ["stretch_i16", "stretch_f16"])
def test_stretch_formats(ctx, oracle, name, fmt):
    n, bs = FIVE_BLOCKS
    data = text(n)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    rows = ctx.export_steps_device(device_model(oracle, name), d_in, bs, fmt, bit=True)
    assert rows.dtype == (torch.int16 if fmt == "stretch_i16" else torch.float16)
    _same(_np(rows), as_format(oracle, expected_p(oracle, name, data, bs, (n, bs)), fmt))


@pytest.mark.parametrize("variant", ["slot_table", "slot_sorted"])
def test_slot_leaf_on_both_of_its_kernels(oracle, variant):
    n, bs = FIVE_BLOCKS
    data = text(n)
    c = w3.Context(0)
    try:
        c.set_variant(variant)
        rows = c.export_steps_device(device_model(oracle, "slot"), torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(), bs, "p_u16")
        _same(_np(rows), expected_p(oracle, "slot", data, bs, (n, bs)))
    finally:
        c.close()


@pytest.mark.parametrize("name", ["o0_apm", "o012_apm2"])
def test_staged_pieces_iter_steps_and_both_store_forms_give_the_same_rows(oracle, name):
    n, bs = FIVE_BLOCKS
    data = text(n)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    model = device_model(oracle, name)
    want = expected_p(oracle, name, data, bs, (n, bs))
    c = w3.Context(0)
    try:
        one = _np(c.export_steps_device(model, d_in, bs, "p_u16"))
        _same(one, want)
        assert c.steps_profile()["direct_stores"] == 0
        c.set_host_chunk_blocks(2)                      # ragged pieces: 2 + 2 + 1 blocks
        staged = c.export_steps(model, data, bs, "p_u16")
        assert c.timing()["n_parts"] == 3
        _same(staged, one)
        _same(c.export_steps(model, data, bs, "stretch_f16"), as_format(oracle, want, "stretch_f16"))
        c.set_host_chunk_blocks(0)
        _same(c.export_steps(model, data, bs, "p_u16"), one)
        got = []
        for first, rows in c.iter_steps(model, d_in, bs, 2, format="p_u16"):
            assert first == 8 * 2 * bs * len(got)
            got.append(_np(rows).copy())
        assert [len(g) for g in got] == [8 * 2048, 8 * 2048, 8 * 37]
        _same(np.concatenate(got), one)
        c.set_tune(L.W3_TUNE_STEPS_DIRECT)              # the direct store form
        for fmt in ("p_u16", "stretch_i16"):
            _same(_np(c.export_steps_device(model, d_in, bs, fmt)), as_format(oracle, want, fmt))
            assert c.steps_profile()["direct_stores"] == 1
        for n2, bs2 in [(63, 64), (65, 32)]:
            d2 = text(n2)
            _same(_np(c.export_steps_device(model, torch.frombuffer(bytearray(d2), dtype=torch.uint8).cuda(), bs2, "p_u16")),
                  expected_p(oracle, name, d2, bs2, (n2, bs2)))
    finally:
        c.close()


def test_errors_come_before_any_launch(ctx, oracle):
    n, bs = 2048, 1024
    data = text(n)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    spec = device_model(oracle, "o012_apm").spec()
    cols = ctx.steps_layout(spec, "p_u16", True)["n_cols"]
    buf = torch.full((8 * n * cols * 2 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0

    def call(sp, ptr, cap, fmt=L.W3_STEPS_P_U16, flags=L.W3_STEPS_COL_BIT, nn=n, b=bs):
        return ctx.lib.w3_export_steps_device(ctx.h, C.byref(sp), C.c_void_p(d_in.data_ptr()), nn, b, fmt, flags, C.c_void_p(ptr), cap, None)
    need = 8 * n * cols * 2
    assert call(spec, buf.data_ptr() + 8, need) == L.W3_E_INVALID                  # misaligned rows
    assert call(spec, buf.data_ptr(), need - 1) == L.W3_E_NOSPACE                  # short rows_cap
    assert b"bytes needed" in ctx.lib.w3_last_error(ctx.h)
    assert call(spec, buf.data_ptr(), need, fmt=3) == L.W3_E_INVALID
    assert call(spec, buf.data_ptr(), need, flags=2) == L.W3_E_INVALID
    assert call(spec, buf.data_ptr(), need, nn=0) == L.W3_OK                       # nothing to do
    # outside twophase_supported: the message of w3_predict_blocks
    assert call(spec, buf.data_ptr(), need, nn=7) == L.W3_E_UNSUPPORTED
    msg = ctx.lib.w3_last_error(ctx.h)
    with pytest.raises(w3.W3Error):
        ctx.predict_blocks(device_model(oracle, "o012_apm"), data[:7], bs)
    assert ctx.lib.w3_last_error(ctx.h) == msg
    assert call(spec, buf.data_ptr(), 1 << 40, b=(1 << 24) + 1) == L.W3_E_UNSUPPORTED
    assert bool((buf == 0x5A).all())                                               # nothing was written
    # while a job is in flight
    d_out = torch.empty(int(ctx.lib.w3_max_compressed_size(n, bs)), dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    job = ctx.encode_submit(spec, d_in, bs, d_out, d_lens, d_total)
    try:
        assert call(spec, buf.data_ptr(), need) == L.W3_E_INVALID
        assert b"in flight" in ctx.lib.w3_last_error(ctx.h)
    finally:
        ctx.encode_wait(job)
    assert bool((buf == 0x5A).all())
    assert call(spec, buf.data_ptr(), need) == L.W3_OK
    assert not bool((buf[:need] == 0x5A).all()) and bool((buf[need:] == 0x5A).all())


@pytest.mark.parametrize("name", ["o0_apm", "o012_apm"])
def test_a_misordered_lds_add_is_caught_and_the_rows_are_still_the_oracles(oracle, name):
    """The value-swap hook of tests/test_gpu_lds_fault.py under the export: with every block sampled (W3_OPT_VERIFY 256) the
    re-prediction sees the fault, the call predicts again on the ballot path, and the rows are the oracle's.  o0_apm: the verification
    has to run before the stage rewrites the single leaf's stream in place."""
    n, bs = FIVE_BLOCKS
    data = text(n)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    model = device_model(oracle, name)
    want = expected_p(oracle, name, data, bs, (n, bs))
    c = w3.Context(0)
    try:
        c.set_verify(256)
        _same(_np(c.export_steps_device(model, d_in, bs, "p_u16")), want)       # clean run: nothing found
        assert c.timing()["n_lds_faults"] == 0
        c.set_variant("inject_lds_fault")
        rows = c.export_steps_device(model, d_in, bs, "p_u16")
        assert c.timing()["n_lds_faults"] >= 1 and c.steps_profile()["n_lds_faults"] >= 1
        _same(_np(rows), want)
        rows = c.export_steps_device(model, d_in, bs, "p_u16")                   # the context stays on the ballot path
        assert c.timing()["n_lds_faults"] == 0
        _same(_np(rows), want)
    finally:
        c.close()
