"""The slot-state leaf's Cell states, k_slot's pipeline cases and the sorted replay's cases, in every kernel that restates the leaf,
on the inputs of tests/slot_census.py (tests/test_slot_census_cpu.py shows that they reach every named kind and that a model wrong
in one kind predicts differently on them).  The truth is the oracle.  Per input and layout: the leaf's predictions step for step
from the sorted replay (w3_slot2.h) and from k_slot (w3_slot.h); the streams from the default path, k_slot, k_cm_staged, k_cm and
the path without LDS atomics; the decode through k_decode_spec in its four forms and through both lane-per-block kernels — for the
leaf alone and for BestOfTwo(Order0, leaf) below one APM."""
import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests import slot_census as sc
from tests.synth import markov_text

pytestmark = pytest.mark.gpu

TEXT = markov_text(3 * 4096, seed=61)
BS = 4096


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def leaf_alone(m, order, log_cells):
    return m.SlotModel(order, log_cells)


def leaf_below_apm(m, order, log_cells):
    return m.APM(m.BestOfTwoModel(m.Order0(), m.SlotModel(order, log_cells)))


SANDWICHES = {"leaf": leaf_alone, "order0_leaf_apm": leaf_below_apm}


def oracle_predict(oracle, mk, data, bs):
    return np.concatenate([oracle.predict_all(mk(oracle), data[o:o + bs]) for o in range(0, len(data), bs)])


def where(name, data, bs, first, step):
    """the failure message of a step that differs: its block, and, inside the census input, what the model says of the event"""
    blk, byte = divmod(step // 8, bs)
    s = 8 * byte + step % 8
    text = "step %d = block %d step %d" % (step, blk, s)
    if name is not None and blk == first:
        text += ": " + sc.describe(*sc.block(name), s)
    return text


def check_predictions(ctx, oracle, mk, data, bs, name=None, first=0, variants=("slot_sorted", "slot_table"), sorted_runs=True):
    want = oracle_predict(oracle, mk, data, bs)
    for variant in variants:
        ctx.set_variant(variant)
        try:
            got = ctx.predict_blocks(mk(w3), data, bs)
            # which kernel predicted: the replay sets the count of table launches to 0, k_slot adds one per batch of tables
            launches = ctx.timing()["n_slot_launches"]
        finally:
            ctx.set_variant()
        assert (launches == 0) == (variant == "slot_sorted" and sorted_runs), "%s: %d table launches" % (variant, launches)
        bad = np.flatnonzero(got != want)
        assert not len(bad), "%s, %d steps differ, the first: got %d, want %d at %s" % (
            variant, len(bad), got[bad[0]], want[bad[0]], where(name, data, bs, first, int(bad[0])))


def check_streams(ctx, oracle, mk, data, bs, sorted_runs=True, twophase=True):
    """-> (streams, lens) of the oracle, after every encode path gave exactly them"""
    want, wlens = oracle.encode_blocks(mk(oracle), data, bs, nthreads=8)

    def same(what, path=None):
        out, lens = ctx.encode_blocks(mk(w3), data, bs)
        assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes(), what
        if path is not None:
            assert ctx.timing()["path"] == path, what

    same("default path", 2 if twophase else 1)
    for variant in ("slot_sorted", "slot_table", "no_lds_atomics"):
        ctx.set_variant(variant)
        try:
            same(variant, 2 if twophase else 1)
            if twophase:
                # which kernel ran the leaves: the replay has no table launches, k_slot at least one.  A call that found the replay's
                # sort out of order is coded again on k_slot, and says nothing about the replay.
                t = ctx.timing()
                assert t["n_lds_faults"] == 0, variant + ": an order fault was reported"
                assert (t["n_slot_launches"] == 0) == (variant == "slot_sorted" and sorted_runs), (variant, t["n_slot_launches"])
        finally:
            ctx.set_variant()
    ctx.set_path("generic")
    try:
        same("generic path (k_cm_staged)", 1)
        ctx.set_variant("cm_unstaged")
        same("generic path, cm_unstaged (k_cm)", 1)
    finally:
        ctx.set_variant()
        ctx.set_path("auto")
    return want, wlens


def check_decodes(ctx, mk, data, bs, out, lens):
    def back(what):
        assert ctx.decode_blocks(mk(w3), out, lens, bs, len(data)).tobytes() == bytes(data), what

    back("k_decode_spec")
    for tune, what in ((16384, "two-bit groups"), (262144, "nibble-major table formats"), (524288, "general kernel")):
        ctx.set_tune(tune)
        try:
            back("k_decode_spec, " + what)
        finally:
            ctx.set_tune(0)
    for variant in (("decode_lane",), ("decode_lane", "cm_unstaged")):
        ctx.set_variant(*variant)
        try:
            back("lane-per-block decoder " + " ".join(variant))
        finally:
            ctx.set_variant()


def check_all(ctx, oracle, order, log_cells, data, bs, name=None, first=0, sorted_runs=True):
    twophase = len(data) >= 8        # (shorter inputs are coded by the lane-per-block kernels alone, and have no predict call)
    for sname, sandwich in SANDWICHES.items():
        def mk(m):
            return sandwich(m, order, log_cells)
        try:
            if twophase:
                check_predictions(ctx, oracle, mk, data, bs, name if sname == "leaf" else None, first, sorted_runs=sorted_runs)
            out, lens = check_streams(ctx, oracle, mk, data, bs, sorted_runs, twophase)
            check_decodes(ctx, mk, data, bs, out, lens)
        except AssertionError as e:
            raise AssertionError("%s, SlotModel(%d, %d) as %s, %d bytes in blocks of %d: %s" % (name, order, log_cells, sname, len(data), bs, e)) from None


@pytest.mark.parametrize("name", list(sc.SMALL_INPUTS))
def test_census_input_as_a_single_block(ctx, oracle, name):
    data, order, log_cells = sc.block(name)
    check_all(ctx, oracle, order, log_cells, data, BS, name, 0)
    if len(data) < 8:       # k_slot and the replay meet a block this short only as the ragged last one
        check_all(ctx, oracle, order, log_cells, TEXT[:BS] + data, BS, name, 1)


@pytest.mark.parametrize("name", list(sc.SMALL_INPUTS))
def test_census_input_between_two_blocks(ctx, oracle, name):
    """the second of three blocks: text before it, a short ragged block after it (tables, open Cells and lanes of the neighbours
    must not leak into it, nor its own into them)"""
    data, order, log_cells = sc.block(name)
    bs = len(data)
    before = max(1, -(-8 // bs))      # (blocks of text before it: one, or as many as make 8 bytes)
    whole = TEXT[:before * bs] + data + TEXT[5000:5000 + min(37, (bs + 1) // 2)]
    check_all(ctx, oracle, order, log_cells, whole, bs, name, before)


@pytest.mark.parametrize("name", sc.PIPELINE_INPUTS)
def test_pipeline_input_in_65_lanes(ctx, oracle, name):
    """65 blocks of 512 bytes: a full wavefront of k_slot whose lanes meet c[e+2] = c[e] at different steps, and a second one with
    one short lane and 63 mirrored ones"""
    _, order, log_cells = sc.block(name)
    check_all(ctx, oracle, order, log_cells, sc.layout_of(name), 512)


# ---- shapes no other test runs: one directed input and 12 KiB of text, in 4 KiB blocks -------------------------------------------------
def with_text(name):
    data = sc.block(name)[0]
    assert len(data) == BS
    return data + TEXT


@pytest.mark.parametrize("shape,name", [((1, 6), "random_cells64"), ((2, 7), "random_cells128"), ((2, 5), "alphabet12_cells4")])
def test_tables_of_32_64_and_128_cells(ctx, oracle, shape, name):
    """2^6 Cells: one replay wavefront with exactly one fine bin per lane; 2^7: two wavefronts; 2^5: half the lanes idle"""
    check_all(ctx, oracle, shape[0], shape[1], with_text(name), BS)


def test_table_of_2_to_the_17_cells_steps_aside(ctx, oracle):
    """above 2^16 Cells the replay's 16-bit sort key does not hold the Cell: slot_sorted must still give the oracle's output (on k_slot)"""
    check_all(ctx, oracle, 2, 17, with_text("alphabet40_cells4096"), BS, sorted_runs=False)


def many_leaves(m, shapes):
    t = m.SlotModel(*shapes[0])
    for shape in shapes[1:]:
        t = m.BestOfTwoModel(t, m.SlotModel(*shape))
    return t


EIGHT = [(1, 4), (2, 12), (0, 2), (3, 8), (1, 6), (4, 16), (2, 7), (7, 10)]


def test_eight_slot_leaves(ctx, oracle):
    """the most that k_cm_staged, k_decode_spec and one launch of k_slot / of the replay take, of mixed orders and sizes"""
    data = with_text("runs_shared_cell")

    def mk(m):
        return many_leaves(m, EIGHT)
    check_predictions(ctx, oracle, mk, data, BS)
    out, lens = check_streams(ctx, oracle, mk, data, BS)
    check_decodes(ctx, mk, data, BS, out, lens)


def test_nine_slot_leaves_take_the_generic_path(ctx, oracle):
    """one more than the two-phase kernels, k_cm_staged and k_decode_spec take: the encode runs on k_cm (timing path 1 whatever is
    asked for) and the decode on the lane-per-block k_cm.  Which decode kernel ran cannot be observed from here: a decode call
    fills no timing and reports nothing but its bytes, so the test asserts only that the default decode and decode_lane both
    return the input; that k_decode_spec and k_cm_staged step aside above eight slot leaves is read in the host code
    (decode_spec_covers, lane_launch)."""
    data = with_text("runs_shared_cell")

    def mk(m):
        return many_leaves(m, EIGHT + [(2, 5)])
    want, wlens = oracle.encode_blocks(mk(oracle), data, BS, nthreads=8)
    for variant in ((), ("slot_sorted",), ("cm_unstaged",)):
        ctx.set_variant(*variant)
        try:
            out, lens = ctx.encode_blocks(mk(w3), data, BS)
            assert ctx.timing()["path"] == 1, variant
        finally:
            ctx.set_variant()
        assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes(), variant
    with pytest.raises(w3.W3Error):
        ctx.predict_blocks(mk(w3), data, BS)      # (the two-phase predict kernels do not cover it: an error, not another path)
    for variant in ((), ("decode_lane",)):
        ctx.set_variant(*variant)
        try:
            assert ctx.decode_blocks(mk(w3), out, lens, BS, len(data)).tobytes() == bytes(data), variant
        finally:
            ctx.set_variant()
