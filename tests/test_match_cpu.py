"""The match-model leaf (W3_HIST_MATCH) on the CPU: tests/match_ref.py, the restatement every GPU test of the leaf compares with.  First
steps worked out by hand, digests that pin the definition (tests/golden/match_streams.json), the states directed inputs reach, mutants of
the definition that must predict differently, the round trip through the oracle's coder with the bit-by-bit model, and the one reason
the leaf exists: fewer coded bytes than the same mixer without it."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

from tests import apm_census as ac
from tests import match_ref as mt
from tests import mixer_ref as mr
from tests.synth import markov_text

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_streams.json")
GOLDEN_MODELS = {
    "leaf_2_8": ((("match", 2, 8),), "leaf", ()),
    "leaf_3_12": ((("match", 3, 12),), "leaf", ()),
    "leaf_4_16": ((("match", 4, 16),), "leaf", ()),
    "o012m_mix": (mt.O012M, "mix", ()),
    "o0m_tree_apm01": ((("o0",), mt.MATCH), "tree", ((ac.ORDER0, 7), (ac.ORDER1, 6))),
}


def golden_inputs():
    d = dict(mt.DIRECTED)
    d["markov_4096"] = markov_text(4096, seed=7)
    return d


def golden_entry(orc, model, data):
    leaves, combine, stages = GOLDEN_MODELS[model]
    p = mt.predict_block(orc, leaves, data, combine, stages=stages)
    stream, bits = mr.code_block(orc, p, data)
    return [len(stream), bits, hashlib.sha256(np.array(p, dtype="<u2").tobytes()).hexdigest(), hashlib.sha256(stream).hexdigest()]


def test_counter_is_the_oracles(oracle):
    """the Python Counter against the oracle's Order0 (2^11 Counters over the same contexts a raw 8-bit history gives)"""
    data = bytes(3000) + b"\xff" * 3000 + markov_text(2000, seed=5)
    want = oracle.predict_all(oracle.Order0(), data).tolist()
    tbl, hist, got = {}, 0, []
    for t in range(8 * len(data)):
        ctx = 0 if t == 0 else ((hist & 255) << 3) | (t & 7)
        c = tbl.setdefault(ctx, mt.Counter())
        got.append(c.p())
        bit = (data[t >> 3] >> (7 - (t & 7))) & 1
        c.update(bit)
        hist = hist << 1 | bit
    assert got == want


def test_first_boundaries_by_hand():
    # "abcabcabd", m = 2, L = 16.  Boundaries 0, 1: no context.  2 ("ab"), 3 ("bc"), 4 ("ca"): empty slots, T_2 records them; 4: the
    # long context "abca" is recorded too.  5: "ab" was at 2 -> c = 2, x[4] = x[1], x[3] = x[0], then the block start: v = 2 = min(CAP, c);
    # e = x[2] = 'c', lq = 2.  The byte at 5 is 'c': all eight keys are (2 << 1) | bit of 'c'.
    x = b"abcabcabd"
    ks = mt.keys(x, 2, 16)
    assert ks[:40] == [0] * 40
    c = ord("c")
    assert ks[40:48] == [(2 << 1) | ((c >> (7 - j)) & 1) for j in range(8)]
    # 6: "bc" was at 3: v = 3 (stopped by the block start); the long "abcb"... is new (v_4 = 0): short stays.  e = x[3] = 'a', byte 'a'.
    assert ks[48:56] == [(3 << 1) | ((ord("a") >> (7 - j)) & 1) for j in range(8)]
    # 7: "ca" at 4, v = 4, and the long "bcab"... first seen at 7: short.  e = x[4] = 'b'.
    assert ks[56:64] == [(4 << 1) | ((ord("b") >> (7 - j)) & 1) for j in range(8)]
    # 8: "ab" most recently at 5 (v = 5 = c), the long "cab" + "a"... "bcab" was recorded at 7?  no: boundary 8's long context is x[4..8) =
    # "bcab", first recorded at 7 as x[3..7) = "abca" -> different strings; whatever the long table holds it is not strictly longer than 5
    # bytes unless it verifies more, and c_long < 5 bounds it.  e = x[5] = 'c', the byte is 'd' = 0x64 against 0x63: bits 0..4 agree
    # (01100), bit 5 differs (0 expected, 1 seen... 'c' = 01100011, 'd' = 01100100): keys for j = 0..5, then 0.
    want = [(5 << 1) | ((c >> (7 - j)) & 1) for j in range(6)] + [0, 0]
    assert ks[64:72] == want
    # the length bucket
    assert [mt.lq_of(v) for v in (1, 15, 16, 19, 20, 31, 32)] == [1, 15, 16, 16, 17, 19, 20]
    assert max(mt.keys(bytes(200), 4, 8)) == (20 << 1) and max(mt.keys(b"\xff" * 200, 4, 8)) == 41


def test_golden_digests(oracle):
    want = json.load(open(GOLDEN))
    inputs = golden_inputs()
    assert sorted(want) == sorted(inputs)
    for iname, data in inputs.items():
        for model in GOLDEN_MODELS:
            assert golden_entry(oracle, model, data) == want[iname][model], (iname, model)


def test_directed_inputs_reach_every_state():
    for data in mt.DIRECTED.values():
        assert len(data) <= 4096
    total = collections.Counter()
    per_config = {}
    for m, L in mt.CONFIGS:
        st = collections.Counter()
        for name in mt.DIRECTED:
            st.update(mt.reached(name, m, L))
        per_config[(m, L)] = st
        total.update(st)
    assert [k for k in mt.STATES if not total[k]] == []
    # what does not depend on a collision is reached under every configuration ...
    needs_collision = {"v_zero", "v_below_m", "short_longer"} | {"v_%d" % v for v in (1, 2, 3)}
    for cfg, st in per_config.items():
        assert [k for k in mt.STATES if k not in needs_collision and not st[k]] == [], cfg
    # ... a collision in the long table only where the tables are small, and v < m needs m > 1 bytes of chance agreement
    assert per_config[(2, 8)]["short_longer"] and per_config[(2, 8)]["v_zero"] and per_config[(2, 8)]["v_1"]
    assert per_config[(4, 16)]["v_below_m"] or per_config[(3, 12)]["v_below_m"]
    # single inputs: a block of zeros makes whole rounds meet one entry, and its compares run into the block start
    z = mt.reached("zeros", 4, 16)
    assert z["round_all_equal"] >= 2 * 62 and z["stopped_by_start"] and z["cap"] and z["expect_1"] == 0
    assert mt.reached("period_64", 4, 16)["cand_64_back"] and mt.reached("period_7", 2, 8)["cand_same_round"]
    mm = mt.reached("mismatch_bits", 4, 16)
    assert all(mm["mismatch_bit_%d" % j] for j in range(8))


_TRUTH = {}


def truth(name, m, L):
    """the definition's stream of a directed input, computed once and shared among the mutants"""
    if (name, m, L) not in _TRUTH:
        _TRUTH[(name, m, L)] = mt.leaf_stream(mt.DIRECTED[name], m, L)
    return _TRUTH[(name, m, L)]


@pytest.mark.parametrize("mutant", mt.MUTANTS)
def test_a_definition_wrong_in_one_behaviour_predicts_differently(mutant):
    differs = []
    for m, L in mt.CONFIGS:
        for name, data in mt.DIRECTED.items():
            if mt.leaf_stream(data, m, L, mutant) != truth(name, m, L):
                differs.append((name, m, L))
    assert differs, mutant


@pytest.mark.parametrize("stages", [(), ((ac.ORDER0, 7), (ac.ORDER1, 6))])
def test_round_trip_and_bit_by_bit_model(oracle, stages):
    data = markov_text(1500, seed=3) + bytes(40) + b"\xff" * 40 + markov_text(300, seed=3)
    leaves = mt.O012 + (("match", 3, 12), ("slot", 2, 10))
    comp, lens, _ = mt.encode_blocks(oracle, leaves, data, 700, stages=stages)
    assert mt.decode_blocks(oracle, leaves, comp, lens, 700, len(data), stages=stages) == data
    blk = data[:700]
    m = mt.Incremental(oracle, leaves, stages=stages)
    got = []
    for byte in blk:
        for j in range(8):
            got.append(m.predict())
            m.update((byte >> (7 - j)) & 1)
    assert got == mt.predict_block(oracle, leaves, blk, stages=stages)


@pytest.mark.parametrize("block_size", [65536, 16384])
def test_the_match_leaf_pays_under_the_mixer(oracle, block_size):
    """coded bytes of order012_match_mix() against order012_mix(), both from the restatement (the prototype's ideal code lengths said
    -4.7 % in 64 KiB blocks and -4.35 % in 16 KiB blocks; DESIGN.md section 4 records the coder's figures)"""
    data = markov_text(65536)
    with_leaf, _, _ = mt.encode_blocks(oracle, mt.O012M, data, block_size)
    without, _, _ = mr.encode_blocks(oracle, mt.O012, data, block_size)
    print("block %d: order012_match_mix %d bytes, order012_mix %d bytes (%+.2f %%)" % (block_size, len(with_leaf), len(without),
                                                                                         100.0 * (len(with_leaf) - len(without)) / len(without)))
    assert len(with_leaf) < len(without)
