"""k_rank_sorted's round kinds, the slice cuts of k_partition / k_partition8 and k_apm1's round classes on the inputs of
tests/rank_census.py, which tests/test_rank_census_cpu.py shows to reach every named state of that code in every leaf form.  The truth
is always the CPU oracle: streams and length table of oracle.encode_blocks byte for byte on the twophase path, and oracle.predict_all
step for step (order1, best012 and the APM over the Order1 records), where a wrong probability is pinned to its step (and, through
rank_census.describe, to its round).
  Every small input is encoded as a single block and as the second of three blocks (a text block before it, a short ragged block behind),
by seven models — Order1, order 2 from scratch, order 2 chained behind Order1, the same beside an ACHistory leaf, and three APM shapes
that run k_apm1 over the Order1 records — under the default kernels and under every alternative implementation of the same step:
the 4-bit partition passes, the order-2 partition from scratch, ballot rounds only, the half-CU instances, and the eight-wavefront
rank instance (staging batches of 4 rounds) through submit / wait.  No call may leave the twophase path or trip the sampled
verification of the LDS adds: a call that does has recovered on the ballot path, and its streams say nothing about the LDS-add rounds.
  The one block of 5,000,000 bytes (records after a latch inside one slice: only a block of more than 64 * 65400 records has them) is
encoded alone, by order1 and best012, default kernels."""
import time

import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests import rank_census as rc
from tests.synth import markov_text
from tests.test_gpu_cm import pair as cm_pair
from tests.test_gpu_parity import _device_bufs, decode_both, pair

pytestmark = pytest.mark.gpu

SMALL = list(rc.SMALL_INPUTS)
LAYOUTS = ["single", "second_of_three"]
MODELS = ["order1", "order2", "best012", "best_ac_wide", "apm1_order1_r6", "apm_chain", "o012_apm"]
# name -> (W3_OPT_VARIANT names, W3_OPT_TUNE bits) of the synchronous calls
VARIANTS = {"default": ((), 0), "partition4": (("partition4",), 0), "no_chained_partition": (("no_chained_partition",), 0),
            "no_lds_atomics": (("no_lds_atomics",), 0), "half_cu": (("half_cu",), 32)}
RANK8_TUNE = 4096 | 32768      # the ordered pair of jobs, rank kernels of eight wavefronts per half CU (as tests/test_gpu_parity.py's test_submit_wait_pipeline)
# models whose predictions are compared step for step -> the leaf forms rank_census.describe reports for a differing step
FORMS_OF = {"order1": ["order1"], "best012": ["order1", "order2_c2_major", "order2_c1_major"], "apm1_order1_r6": ["order1"]}


def models(oracle, name):
    """(device model factory, oracle model factory); the oracle twins of the APM shapes as tests/test_gpu_cm.py builds them"""
    o = oracle
    if name == "apm1_order1_r6":
        return (lambda: w3.APM(w3.Order1(), w3.APM.ORDER1, 6), lambda: o.APM(o.Order1(), o.APM_ORDER1, 6))
    if name == "apm_chain":
        return (lambda: w3.APM(w3.APM(w3.Order1(), 0, 7), 1, 6), lambda: o.APM(o.APM(o.Order1(), 0, 7), 1, 6))
    if name == "o012_apm":
        return cm_pair(oracle, name)
    return pair(oracle, name)


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    c.set_path("twophase")
    yield c
    c.close()


_layouts, _truth, _steps = {}, {}, {}


def layout(name, kind):
    """-> (data, block size, offset of the input's block)"""
    if (name, kind) not in _layouts:
        blk = rc.block(name)
        bs = len(blk)
        _layouts[(name, kind)] = (blk, bs, 0) if kind == "single" else (markov_text(bs, seed=77) + blk + markov_text(max(bs // 3, 5), seed=78), bs, bs)
    return _layouts[(name, kind)]


def truth(oracle, name, kind, model):
    """oracle.encode_blocks, once per input, layout and model"""
    key = (name, kind, model)
    if key not in _truth:
        data, bs, _ = layout(name, kind)
        _truth[key] = oracle.encode_blocks(models(oracle, model)[1](), data, bs, nthreads=8)
    return _truth[key]


def truth_steps(oracle, name, kind, model):
    """oracle.predict_all block by block"""
    key = (name, kind, model)
    if key not in _steps:
        data, bs, _ = layout(name, kind)
        _steps[key] = np.concatenate([oracle.predict_all(models(oracle, model)[1](), data[o:o + bs]) for o in range(0, len(data), bs)])
    return _steps[key]


def configure(ctx, variant):
    names, tune = VARIANTS[variant]
    ctx.set_variant(*names)      # (also re-arms the LDS-add path, should an earlier call have left it)
    ctx.set_tune(tune)


def reset(ctx):
    ctx.set_tune(0)
    ctx.set_variant()


def assert_clean_call(ctx, what):
    t = ctx.timing()
    assert t["path"] == 2, what
    assert t["n_lds_faults"] == 0, (what, "the sampled verification found the LDS-add rounds wrong and the call recovered on the ballot path")


def assert_same(got, want, what):
    assert got[1].tolist() == want[1].tolist(), what
    assert got[0].tobytes() == want[0].tobytes(), what


# ---- streams ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("name", SMALL)
def test_streams_match_the_oracle(ctx, oracle, name, kind):
    import torch
    data, bs, _ = layout(name, kind)
    n, nb = len(data), -(-len(data) // bs)
    try:
        for variant in VARIANTS:
            configure(ctx, variant)
            for model in MODELS:
                got = ctx.encode_blocks(models(oracle, model)[0](), data, bs)
                assert_clean_call(ctx, (name, kind, model, variant))
                assert_same(got, truth(oracle, name, kind, model), (name, kind, model, variant))
        reset(ctx)
        d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        d_out, d_lens, d_total = _device_bufs(n, bs, 1)[0]
        torch.cuda.synchronize()
        ctx.set_tune(RANK8_TUNE)
        for model in MODELS:
            ctx.encode_wait(ctx.encode_submit(models(oracle, model)[0](), d_in, bs, d_out, d_lens, d_total))
            assert_clean_call(ctx, (name, kind, model, "rank8"))
            got = (d_out[: int(d_total.item())].cpu().numpy(), d_lens[:nb].cpu().numpy().astype(np.uint32))
            assert_same(got, truth(oracle, name, kind, model), (name, kind, model, "rank8"))
    finally:
        reset(ctx)


# ---- predictions, step for step ---------------------------------------------------------------------------------------------------------
def explain(name, kind, model, step):
    """the first differing step as block, position and bit, and the round the census puts that record in"""
    data, bs, at = layout(name, kind)
    byte, bit = divmod(int(step), 8)
    b, position = divmod(byte, bs)
    where = "step %d = block %d, position %d, bit %d" % (step, b, position, bit)
    if b * bs != at:
        return where + " (not the input's block)"
    return where + "\n" + "\n".join(rc.describe(data[at:at + bs], form, position) for form in FORMS_OF[model])


@pytest.mark.parametrize("name", SMALL)
def test_predictions_step_for_step(ctx, oracle, name):
    try:
        for kind in LAYOUTS:
            data, bs, _ = layout(name, kind)
            for variant in VARIANTS:
                configure(ctx, variant)
                for model in FORMS_OF:
                    want = truth_steps(oracle, name, kind, model)
                    got = ctx.predict_blocks(models(oracle, model)[0](), data, bs)
                    assert got.shape == want.shape
                    diff = np.flatnonzero(got != want)
                    assert len(diff) == 0, "%s %s %s %s: %d steps differ, the first: %s (got %d, want %d)" % (
                        name, kind, model, variant, len(diff), explain(name, kind, model, diff[0]), got[diff[0]], want[diff[0]])
    finally:
        reset(ctx)


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_decode_round_trip(ctx, oracle, name):
    """the oracle's streams of the three-block layout back through the decoders (all of decode_both's forms up to blocks of 16 KiB, the
    default and the lane-per-block decoder above: a decode is one latency chain per block)"""
    data, bs, _ = layout(name, "second_of_three")
    ctx.set_path("auto")
    try:
        for model in MODELS:
            out, lens = truth(oracle, name, "second_of_three", model)
            back = decode_both(ctx, models(oracle, model)[0](), out, lens, bs, len(data), forms=4 if bs <= 16384 else 2)
            assert back.tobytes() == data, (name, model)
    finally:
        ctx.set_path("twophase")


# ---- records after a latch --------------------------------------------------------------------------------------------------------------
def test_groups_after_a_latch_in_one_slice(ctx, oracle):
    """rank_census.after_latch_block: slice 3 opens with the 66,000 records of group 'e', latches on them, ends that group inside a
    ballot round and goes on with further groups; slice 0 latches on a group of 234,374.  Encode only, default kernels."""
    data = rc.block(rc.LARGE_INPUT)
    bs = len(data)
    reset(ctx)
    t0 = time.perf_counter()
    for model in ("order1", "best012"):
        dev, orc = models(oracle, model)
        got = ctx.encode_blocks(dev(), data, bs)
        assert_clean_call(ctx, model)
        assert_same(got, oracle.encode_blocks(orc(), data, bs), model)
    print("test_groups_after_a_latch_in_one_slice: %.2f s" % (time.perf_counter() - t0))
