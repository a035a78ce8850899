"""k_match_keys (csrc/w3_match.h) and k_predict_wave (csrc/w3_predict_wave.h) with MORE BLOCKS THAN WAVEFRONTS.  Both give a wavefront
a private table in device memory and walk the blocks with a grid stride; the host launches one wavefront per block up to what the chip
holds, so below a few thousand blocks every wavefront takes exactly one.  W3_OPT_WAVE_GRID caps the grid: here one, two or three
wavefronts take hundreds of blocks each, over inputs steered (tests/match_ref.py: tag_blocks) so that the tag bookkeeping — the tag check,
the re-zeroing of both tables when the tag returns to 1 after 255 blocks, positions above bit 16 of an entry — and k_predict_wave's
per-block zeroing decide the result; tests/test_match_tags_cpu.py shows on the CPU that each of them, done wrong, changes these cases.
Everything is integer-exact against the restatement (tests/match_ref.py) or the oracle; every case asserts the grid it ran with
(w3_last_wave_grid), so a hook that did nothing fails."""
import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests import apm_census as ac
from tests import match_ref as mt
from tests import mixer_ref as mr
from tests import wave_ref as wr
from weath3rb0i_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def capped(c, waves, path="twophase"):
    """context manager: the grid cap and the path for the calls inside"""
    class _Cap:
        def __enter__(self):
            c.set_wave_grid(waves)
            c.set_path(path)

        def __exit__(self, *exc):
            c.set_wave_grid(0)
            c.set_path("auto")
    return _Cap()


def leaf_predictions(c, data, bs, waves, m, Ls):
    with capped(c, waves):
        got = c.predict_blocks(w3.MatchModel(m, Ls), data, bs)
        grid = c.last_wave_grid()
    return got.tolist(), grid


# ---- the option and the export ------------------------------------------------------------------------------------------------------------
def test_the_option_and_the_export(ctx):
    assert L.W3_OPT_WAVE_GRID == 16
    assert ctx.lib.w3_ctx_set_option(ctx.h, L.W3_OPT_WAVE_GRID, -1) == L.W3_E_INVALID
    assert ctx.lib.w3_last_wave_grid(None, None) == L.W3_E_INVALID and ctx.lib.w3_last_wave_grid(ctx.h, None) == L.W3_E_INVALID
    c = w3.Context(0)
    try:
        assert c.last_wave_grid() == (0, 0)   # before any call
        data = mt.two_block_waves(5)
        want = mt.predict_blocks(None, (("match", 2, 8),), data, 24, "leaf")
        # a cap above the block count: one wavefront per block, as without it
        got, grid = leaf_predictions(c, data, 24, 64, 2, 8)
        assert grid == (5, 0) and got == want
        got, grid = leaf_predictions(c, data, 24, 0, 2, 8)
        assert grid == (5, 0) and got == want
        # a model without either kernel
        c.set_path("twophase")
        c.encode_blocks(w3.order012_mix(), data, 24)
        assert c.last_wave_grid() == (0, 0)
    finally:
        c.close()


# ---- (a) the leaf's predictions, a wavefront over hundreds of blocks ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mt.TAG_CASES))
def test_the_leafs_predictions_with_more_blocks_than_wavefronts(ctx, name):
    nb, bs, waves, tail, m, Ls = mt.TAG_CASES[name]
    data = mt.tag_case(name)
    want = mt.predict_blocks(None, (("match", m, Ls),), data, bs, "leaf")
    got, grid = leaf_predictions(ctx, data, bs, waves, m, Ls)
    assert grid == (waves, 0)
    assert got == want


def test_wavefronts_with_two_blocks_beside_wavefronts_with_one(ctx):
    data = mt.two_block_waves(70)
    want = mt.predict_blocks(None, (("match", 2, 8),), data, 24, "leaf")
    got, grid = leaf_predictions(ctx, data, 24, 64, 2, 8)
    assert grid == (64, 0)
    assert got == want


# ---- (b) one long block: entry positions above bit 16 ------------------------------------------------------------------------------------
def test_one_long_block_on_both_paths(ctx, oracle):
    x, bs = mt.long_block(), 131072
    stream = mt.leaf_stream(x, 4, 20)
    with capped(ctx, 1):
        got = ctx.predict_blocks(w3.MatchModel(4, 20), x, bs)
        assert ctx.last_wave_grid() == (1, 0)
    assert got.tolist() == stream
    want, bits = mr.code_block(oracle, stream, x)
    for path in ("twophase", "generic"):
        with capped(ctx, 1, path):
            out, lens = ctx.encode_blocks(w3.MatchModel(4, 20), x, bs)
            assert ctx.timing()["path"] == (L.W3_PATH_TWOPHASE if path == "twophase" else L.W3_PATH_GENERIC)
            if path == "twophase":
                assert ctx.last_wave_grid() == (1, 0)
        assert lens.tolist() == [len(want)] and out.tobytes() == want, path


# ---- (c) whole models ----------------------------------------------------------------------------------------------------------------------
A0 = (ac.ORDER0, 7)
MODELS = {
    "order012_match_mix": (mt.O012M, (), w3.order012_match_mix),
    "o0_match_2_8_mix_apm": ((("o0",), ("match", 2, 8)), (A0,), lambda: w3.APM(w3.LogisticMixer([w3.Order0(), w3.MatchModel(2, 8)]), w3.APM.ORDER0, 7)),
}
INPUTS = ["300x40_w1_4_16", "520x24_w1_2_8"]
_REF = {}


def ref(oracle, model, inp):
    if (model, inp) not in _REF:
        leaves, stages, _ = MODELS[model]
        _REF[model, inp] = mt.encode_blocks(oracle, leaves, mt.tag_case(inp), mt.TAG_CASES[inp][1], "mix", stages=stages)
    return _REF[model, inp]


@pytest.mark.parametrize("inp", INPUTS)
@pytest.mark.parametrize("model", sorted(MODELS))
def test_whole_models_with_one_wavefront(ctx, oracle, model, inp):
    import torch
    make, bs, data = MODELS[model][2], mt.TAG_CASES[inp][1], mt.tag_case(inp)
    want, wlens, wbits = ref(oracle, model, inp)
    with capped(ctx, 1):
        out, lens = ctx.encode_blocks(make(), data, bs)
        assert ctx.timing()["path"] == L.W3_PATH_TWOPHASE and ctx.last_wave_grid() == (1, 0)
        bits = ctx.encode_stats(make(), data, bs)
        assert ctx.last_wave_grid() == (1, 0)
    assert lens.tolist() == wlens and out.tobytes() == want, "two-phase path, one wavefront"
    assert bits.tolist() == wbits
    with capped(ctx, 1, "generic"):
        lane, llens = ctx.encode_blocks(make(), data, bs)
        assert ctx.timing()["path"] == L.W3_PATH_GENERIC
    assert llens.tolist() == wlens and lane.tobytes() == want, "lane kernel"
    back = ctx.decode_blocks(make(), out, lens, bs, len(data))
    assert ctx.last_decode_path() == L.W3_PATH_GENERIC and back.tobytes() == data
    # one submitted job
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    d_out = torch.empty(2 * len(data) + 16 * len(wlens) + 4096, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(len(wlens), dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with capped(ctx, 1):
        ctx.encode_wait(ctx.encode_submit(make(), d_in, bs, d_out, d_lens, d_total))
        assert ctx.last_wave_grid() == (1, 0)
    assert d_lens.cpu().numpy().astype(np.uint32).tolist() == wlens
    assert d_out[:int(d_total.item())].cpu().numpy().tobytes() == want


# ---- (d) calls in a row on one context: the tables hold the call before's entries ---------------------------------------------------------
def test_calls_in_a_row_on_one_context():
    nb, bs, waves, tail, m, _ = mt.TAG_CASES["520x24_tail_w1_2_12"]
    data = mt.tag_case("520x24_tail_w1_2_12")
    want = {Ls: mt.predict_blocks(None, (("match", m, Ls),), data, bs, "leaf") for Ls in (12, 16)}
    c = w3.Context(0)
    try:
        for Ls in (12, 12, 16, 12):   # the same data twice; then another table layout and back
            got, grid = leaf_predictions(c, data, bs, 1, m, Ls)
            assert grid == (1, 0)
            fresh = w3.Context(0)
            try:
                alone, grid = leaf_predictions(fresh, data, bs, 1, m, Ls)
            finally:
                fresh.close()
            assert grid == (1, 0)
            assert got == alone == want[Ls], Ls
    finally:
        c.close()


# ---- (e) k_predict_wave: one table, block after block ------------------------------------------------------------------------------------------
_WANT = {}


@pytest.mark.parametrize("waves", [1, 3])
@pytest.mark.parametrize("kind", ["equal", "alternating"])
@pytest.mark.parametrize("leaf", sorted(wr.LEAVES))
def test_predict_wave_with_more_blocks_than_wavefronts(ctx, oracle, leaf, kind, waves):
    lf = wr.LEAVES[leaf]
    data = wr.inputs()[kind]
    if (leaf, kind) not in _WANT:
        _WANT[leaf, kind] = wr.oracle_blocks(oracle, lf, data, wr.BLOCK)
    with capped(ctx, waves):
        got = ctx.predict_blocks(mr.w3_leaf(w3, lf), data, wr.BLOCK)
        assert ctx.last_wave_grid() == (0, waves)
    assert got.tolist() == _WANT[leaf, kind]


def test_several_wave_leaves_report_the_smallest_grid(ctx, oracle):
    """two k_predict_wave leaves and the match leaf in one model, two wavefronts each"""
    data = wr.inputs()["alternating"]
    model = w3.BestOfTwoModel(w3.BestOfTwoModel(mr.w3_leaf(w3, wr.LEAVES["direct_raw"]), w3.MatchModel(2, 8)), mr.w3_leaf(w3, wr.LEAVES["map_keyed"]))
    streams = [wr.oracle_blocks(oracle, wr.LEAVES["direct_raw"], data, wr.BLOCK), mt.predict_blocks(None, (("match", 2, 8),), data, wr.BLOCK, "leaf"),
               wr.oracle_blocks(oracle, wr.LEAVES["map_keyed"], data, wr.BLOCK)]
    with capped(ctx, 2):
        got = ctx.predict_blocks(model, data, wr.BLOCK)
        assert ctx.last_wave_grid() == (2, 2)
    assert got.tolist() == mt.tree(streams)
