"""The logistic mixer node (W3_NODE_MIX) on the CPU: tests/mixer_ref.py, the restatement every GPU test of the node compares with.  First
steps worked out by hand, digests that pin the definition (tests/golden/mixer_streams.json), the round trip through the oracle's coder,
the states directed inputs reach (every clamp of the step, every ORDER0 row), mutants of the step that must predict differently, and
the one reason the node exists: fewer bits than the BestOfTwo tree over the same leaves."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

from tests import apm_census as ac
from tests import mixer_ref as mr
from tests.synth import markov_text

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixer_streams.json")
O012 = (("o0",), ("o1",), ("on", 27, 3))
GOLDEN_MODELS = {
    "o01_order0_r4": (mr.DIRECTED_LEAVES, mr.ORDER0, 4, ()),
    "o012_order0_r14": (O012, mr.ORDER0, 14, ()),
    "o012_one_r16": (O012, mr.ONE, 16, ()),
    "o012_order0_r14_apm01": (O012, mr.ORDER0, 14, ((ac.ORDER0, 7), (ac.ORDER1, 6))),
}


def golden_inputs():
    d = dict(mr.DIRECTED)
    d["markov_4096"] = markov_text(4096, seed=7)
    return d


def golden_entry(orc, model, data):
    leaves, select, rate, stages = GOLDEN_MODELS[model]
    p = mr.predict_block(orc, leaves, data, select, rate, stages)
    stream, bits = mr.code_block(orc, p, data)
    return [len(stream), bits, hashlib.sha256(np.array(p, dtype="<u2").tobytes()).hexdigest(), hashlib.sha256(stream).hexdigest()]


def test_first_steps_by_hand():
    # Leaves whose stretch is 0 (p = 32752 .. 32767: squash(0) = 32768 >= 16 * 2047 + 8): dot 0, p = squash(0) = 32768, err = +-32768,
    # every update (0 * err + round) >> rate = 0 — the weights stay.
    assert ac.STRETCH[32767 >> 4] == 0 and ac.SQUASH[2047] == 32768
    for n in (2, 3, 8):
        w = [65536 // n] * n
        s = [0] * n
        assert mr.predict_d(w, s) == 0
        for bit in (0, 1):
            mr.train(w, s, bit, 32768, 4)
        assert w == [65536 // n] * n
    assert mr.mix([[32767] * 8, [32760] * 8], b"\xa5", mr.ORDER0, 4) == [32768] * 8
    # p = 32768 itself is one bucket higher: stretch = the smallest d with squash(d) >= 16 q + 8 = 32776, which is 1 (squash(1) = 32832).
    # Two leaves: dot = 2 * ((32768 * 1) >> 8) = 256, d = 1, p = 32832; bit 1 at rate 4: err = 32704, (1 * 32704 + 8) >> 4 = 2044.
    # Three leaves: 3 * (21845 >> 8) = 255, d = 0, p = 32768, err = 32768, +2048.  Eight: 8 * (8192 >> 8) = 256, d = 1, +2044.
    assert ac.STRETCH[32768 >> 4] == 1 and ac.SQUASH[2048] == 32832
    for n, d, dw in ((2, 1, 2044), (3, 0, 2048), (8, 1, 2044)):
        w = [65536 // n] * n
        assert mr.predict_d(w, [1] * n) == d
        mr.train(w, [1] * n, 1, ac.SQUASH[2047 + d], 4)
        assert w == [65536 // n + dw] * n
    assert mr.mix([[32768] * 8, [32768] * 8], b"\xa5", mr.ORDER0, 4) == [32832] * 8   # eight different rows, each at its first step
    # one further step, two leaves at p = 49152 and 20480, weights 32768 each, rate 4, bit 1
    s = [ac.STRETCH[49152 >> 4], ac.STRETCH[20480 >> 4]]
    assert s == [282, -201] and ac.SQUASH[2047 + 282] >= 49152 + 8 > ac.SQUASH[2047 + 281]
    w = [32768, 32768]
    # (32768 * 282) >> 8 = 36096, (32768 * -201) >> 8 = -25728; dot = 10368; d = 40
    assert mr.predict_d(w, s) == 40
    p = ac.SQUASH[2047 + 40]
    assert p == 35323
    # err = 65536 - 35323 = 30213; 282 * 30213 + 8 = 8520074, >> 4 = 532504 -> w0 = 565272;
    # -201 * 30213 + 8 = -6072805, >> 4 = -379551 (floor: -379550.3) -> w1 = -346783
    mr.train(w, s, 1, p, 4)
    assert w == [565272, -346783]
    # the next step clamps both ways: 2047 * 65514 >> 4 moves either weight past WMAX
    mr.train(w, [2047, -2047], 1, 22, 4)
    assert w == [mr.WMAX, -mr.WMAX]


def test_golden_digests(oracle):
    want = json.load(open(GOLDEN))
    inputs = golden_inputs()
    assert sorted(want) == sorted(inputs)
    for iname, data in inputs.items():
        for model in GOLDEN_MODELS:
            assert golden_entry(oracle, model, data) == want[iname][model], (iname, model)


@pytest.mark.parametrize("select", [mr.ONE, mr.ORDER0])
@pytest.mark.parametrize("stages", [(), ((ac.ORDER0, 7),), ((ac.ORDER0, 7), (ac.ORDER1, 6))])
def test_round_trip_and_bit_by_bit_model(oracle, select, stages):
    data = markov_text(1500, seed=3) + bytes(40) + b"\xff" * 40
    leaves = O012 + (("slot", 2, 10),)
    comp, lens, _ = mr.encode_blocks(oracle, leaves, data, 700, select, 14, stages)
    assert mr.decode_blocks(oracle, leaves, comp, lens, 700, len(data), select, 14, stages) == data
    # the decoder's bit-by-bit composition predicts what the stream composition (apm_census.stage behind mix) predicts
    blk = data[:700]
    m = mr.Incremental(oracle, leaves, select, 14, stages)
    got = []
    for byte in blk:
        for j in range(8):
            got.append(m.predict())
            m.update((byte >> (7 - j)) & 1)
    assert got == mr.predict_block(oracle, leaves, blk, select, 14, stages)


def test_directed_inputs_reach_every_clamp(oracle):
    for name in ("zeros_then_ff00", "runs_00_ff"):
        states, _ = mr.reached(oracle, name)
        assert all(states[k] > 0 for k in mr.STATES), (name, dict(states))
    states, _ = mr.reached(oracle, "zeros")
    assert states["d_lo"] > 0 and states["w_max"] > 0 and states["d_hi"] == 0
    states, _ = mr.reached(oracle, "ones")
    assert states["d_hi"] > 0 and states["w_max"] > 0 and states["d_lo"] == 0
    for data in mr.DIRECTED.values():
        assert len(data) <= 4096


def test_ramp_visits_every_order0_row(oracle):
    _, rows = mr.reached(oracle, "ramp")
    assert rows == set(range(1, 256))


@pytest.mark.parametrize("mutant", mr.MUTANTS)
def test_a_step_wrong_in_one_behaviour_predicts_differently(oracle, mutant):
    differs = []
    for name, data in mr.DIRECTED.items():
        streams = mr.leaf_streams(oracle, mr.DIRECTED_LEAVES, data)
        if mr.mix(streams, data, mr.ORDER0, 4, mutant=mutant) != mr.mix(streams, data, mr.ORDER0, 4):
            differs.append(name)
    assert differs, mutant


def test_the_mixer_beats_the_selection_tree(oracle):
    """from the reference's parts alone: ACStats bits of the mixer over Order0, Order1, OrderN(27, 3) against BestOfTwo over the same leaves"""
    data = markov_text(32768)
    _, _, bits = mr.encode_blocks(oracle, O012, data, len(data), mr.ORDER0, 14)
    tree = oracle.BestOfTwoModel(oracle.BestOfTwoModel(oracle.Order0(), oracle.Order1()), oracle.OrderN(27, 3))
    tree_bits = oracle.encode_stats_bits(tree, data)
    print("mixer %d bits, BestOfTwo tree %d bits" % (bits[0], tree_bits))
    assert bits[0] < tree_bits
