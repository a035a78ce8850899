"""The APM stage's states, k_apm0's and k_apm1's schedules and the leaf mixer's states in every kernel that restates them, on the inputs
of tests/apm_census.py (tests/test_apm_census_cpu.py shows that they reach every named state for every stage form and that a model
wrong in one behaviour predicts differently on them).  The truth is the oracle.  Per input and layout: every stage's predictions step
for step from k_apm0 / k_apm1; the streams from the default two-phase path, the path without LDS atomics, k_cm_staged / k_cm_nl and
k_cm; the decode through k_decode_spec in its four forms (chains of at most two stages, and the two-stage prefix of longer ones)
and through the lane-per-block kernels (every chain)."""
import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests import apm_census as ac
from tests.synth import markov_text

pytestmark = pytest.mark.gpu

TEXT = markov_text(2 * 8192 + 64, seed=71)


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def blocks_of(data, bs):
    return [data[o:o + bs] for o in range(0, len(data), bs)]


def where(name, stage_index, bs, first, step):
    """the failure message of a step that differs: its block, and, inside the census input, what the model says of the step"""
    blk, byte = divmod(step // 8, bs)
    s = 8 * byte + step % 8
    text = "step %d = block %d step %d" % (step, blk, s)
    if name is not None and blk == first and stage_index >= 0:
        text += ": " + ac.describe(name, stage_index, s)
    return text


def check_predictions(ctx, oracle, leaves, stages, data, bs, name=None, first=0):
    """every chain prefix (from the leaves alone, where there is something to mix) against the oracle"""
    for k in range(0 if len(leaves) > 1 else 1, len(stages) + 1):
        want = np.concatenate([oracle.predict_all(ac.build(oracle, leaves, stages[:k]), b) for b in blocks_of(data, bs)])
        got = ctx.predict_blocks(ac.build(w3, leaves, stages[:k]), data, bs)
        bad = np.flatnonzero(got != want)
        assert not len(bad), "stage %d of %d (%s): %d steps differ, the first: got %d, want %d at %s" % (
            k, len(stages), "the mixed leaves" if k == 0 else "ORDER%d, rate %d" % stages[k - 1], len(bad), got[bad[0]], want[bad[0]],
            where(name, k - 1, bs, first, int(bad[0])))


def check_streams(ctx, oracle, leaves, stages, data, bs):
    """-> (streams, lens) of the oracle, after every encode path gave exactly them"""
    want, wlens = oracle.encode_blocks(ac.build(oracle, leaves, stages), data, bs, nthreads=8)

    def same(what, path):
        out, lens = ctx.encode_blocks(ac.build(w3, leaves, stages), data, bs)
        assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes(), what
        assert ctx.timing()["path"] == path, what

    same("default path", 2)
    ctx.set_variant("no_lds_atomics")
    try:
        same("no_lds_atomics", 2)
    finally:
        ctx.set_variant()
    ctx.set_path("generic")
    try:
        same("generic path (k_cm_staged / k_cm_nl)", 1)
        ctx.set_variant("cm_unstaged")
        same("generic path, cm_unstaged (k_cm)", 1)
    finally:
        ctx.set_variant()
        ctx.set_path("auto")
    return want, wlens


def check_decode_spec(ctx, leaves, stages, data, bs, out, lens):
    def back(what):
        assert ctx.decode_blocks(ac.build(w3, leaves, stages), out, lens, bs, len(data)).tobytes() == bytes(data), what

    back("k_decode_spec")
    for tune, what in ((16384, "two-bit groups"), (262144, "nibble-major table formats"), (524288, "general kernel")):
        ctx.set_tune(tune)
        try:
            back("k_decode_spec, " + what)
        finally:
            ctx.set_tune(0)


def check_decode_lane(ctx, leaves, stages, data, bs, out, lens):
    for variant in (("decode_lane",), ("decode_lane", "cm_unstaged")):
        ctx.set_variant(*variant)
        try:
            assert ctx.decode_blocks(ac.build(w3, leaves, stages), out, lens, bs, len(data)).tobytes() == bytes(data), "lane-per-block decoder " + " ".join(variant)
        finally:
            ctx.set_variant()


def check_all(ctx, oracle, leaves, stages, data, bs, name=None, first=0):
    try:
        check_predictions(ctx, oracle, leaves, stages, data, bs, name, first)
        out, lens = check_streams(ctx, oracle, leaves, stages, data, bs)
        check_decode_lane(ctx, leaves, stages, data, bs, out, lens)
        if len(stages) > 2:          # k_decode_spec takes two stages: the chain's first two, which are a model of their own
            stages = stages[:2]
            out, lens = oracle.encode_blocks(ac.build(oracle, leaves, stages), data, bs, nthreads=8)
        check_decode_spec(ctx, leaves, stages, data, bs, out, lens)
    except AssertionError as e:
        raise AssertionError("%s, %d leaves, stages %s, %d bytes in blocks of %d: %s" % (name, len(leaves), stages, len(data), bs, e)) from None


@pytest.mark.parametrize("name", list(ac.INPUTS))
def test_census_input_as_a_single_block(ctx, oracle, name):
    data, leaves, stages = ac.block(name)
    check_all(ctx, oracle, leaves, stages, data, len(data), name, 0)


@pytest.mark.parametrize("name", list(ac.INPUTS))
def test_census_input_between_two_blocks(ctx, oracle, name):
    """the second of three blocks: text before it, a short ragged block after it (the tables, the hand-over word and the lanes of the
    neighbours must not leak into it, nor its own into them)"""
    data, leaves, stages = ac.block(name)
    bs = len(data)
    check_all(ctx, oracle, leaves, stages, TEXT[:bs] + data + TEXT[8192:8192 + 37], bs, name, 1)


@pytest.mark.parametrize("name,length,nblocks", ac.SHAPES)
def test_launch_shapes_of_k_apm0(ctx, oracle, name, length, nblocks):
    """the FAST form and the ragged ones (a last pair with one lane, an empty round), every exit of the batch loop for both wavefronts
    of a block (1 .. 7 batches), a full workgroup and one with three idle table slots"""
    _, leaves, stages = ac.block(name)
    check_all(ctx, oracle, leaves, stages, ac.shape_data(name, length, nblocks), length)


EIGHTH = ("on", 22, 3)
CODERS = ["x5", "x3", "x2", "fast", "robust"]


@pytest.mark.parametrize("nleaves", [4, 5, 6, 8])
def test_the_other_leaf_counts_of_k_apm0(ctx, oracle, nleaves):
    """k_apm0<L> for the L the census does not use: the mixer input, single and in three blocks of which the last is ragged"""
    data = ac.block("alphabet4.L7")[0]
    leaves = (ac.L7 + [EIGHTH])[:nleaves]
    for d, bs in ((data, len(data)), (data + data[:1000], 1250)):
        check_predictions(ctx, oracle, leaves, [(0, 2)], d, bs)
        check_streams(ctx, oracle, leaves, [(0, 2)], d, bs)


@pytest.mark.parametrize("name", ["alphabet4.L2", "alphabet4.L3", "ramp.o0"])
def test_mixer_states_in_the_coders(ctx, oracle, name):
    """models without an APM: the coders mix the leaves themselves (opinion_mix2): every coder kernel, the robust one by name and
    through the hand-back of a lowered accumulator limit.  (What the limit hands back depends on the pending-bit runs of the input,
    which nothing here steers: on an MI355X 2 of the 7 blocks of alphabet4.L3 and none of the other two inputs'; the count is printed.
    The robust coder by name codes every block.)"""
    data, leaves, _ = ac.block(name)
    leaves = leaves[:3]
    whole = data + TEXT[:8 * 1024 + 37]       # (text behind it: blocks that the lowered limit hands to the robust coder)
    bs = len(data)
    want, wlens = oracle.encode_blocks(ac.build(oracle, leaves, []), whole, bs, nthreads=8)

    def same(what):
        out, lens = ctx.encode_blocks(ac.build(w3, leaves, []), whole, bs)
        assert ctx.timing()["path"] == 2, what
        assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes(), what
        return out, lens

    out, lens = same("default coder")
    try:
        for mode in CODERS:
            ctx.set_coder(mode)
            same("coder " + mode)
    finally:
        ctx.set_coder("x4")
    ctx.set_acc_limit(19)
    try:
        same("accumulator limit 19")
        recoded = ctx.timing()["n_recoded_blocks"]
        print("n_recoded_blocks %s: %d of %d" % (name, recoded, len(wlens)))
    finally:
        ctx.set_acc_limit(46)
    assert ctx.decode_blocks(ac.build(w3, leaves, []), out, lens, bs, len(whole)).tobytes() == whole
    check_predictions(ctx, oracle, leaves, [], whole, bs)
