"""The property the sixteen-lane decoder's mixer rests on (csrc/w3_decode_spec.h, MIX), on the restatement alone: with the weight set
selected by the partial byte (ORDER0) the steps of a nibble use four different rows, none of which the next nibble uses, and a row comes
back after 8 steps at the earliest — so the 15 nodes of a nibble's tree can take their dot products side by side from the weights as they
stand when the nibble starts, and the path's stores need no fence before the next nibble's loads.  With a single weight set (ONE) the
same check fails at the first step: every bit trains the row the next bit reads.  From the `rows` log of tests/mixer_ref.mix."""
from tests import mixer_ref as mr
from tests.synth import lcg_text, markov_text
from weath3rb0i_amd import _lib as L

TEXT = markov_text(6000, seed=23) + lcg_text(1200, seed=5) + bytes(300) + b"\xff" * 300
INPUTS = dict(mr.DIRECTED, text=TEXT)
BLOCK_SIZES = (1, 7, 9, 512, 4096)


class RowLog(list):
    """what mr.mix takes as `rows`: it calls add(c0) once per step, in step order"""
    add = list.append


def row_log(block, select):
    """the weight row of every step of the block: mr.mix logs the partial byte c0 of the step; the row is c0 under ORDER0 and 0 under ONE
    (mr.mix's `w[c0 if select == ORDER0 else 0]`).  The rows do not depend on what the leaves predict: two constant streams stand in."""
    log = RowLog()
    n = 8 * len(block)
    mr.mix([[32768] * n, [20000] * n], block, select, 14, rows=log)
    assert len(log) == n
    return [c0 if select == mr.ORDER0 else 0 for c0 in log]


def first_violation(rows):
    """the first step at which the decoder's assumptions break, or None: the four rows of a nibble distinct, no row of a nibble in the
    next nibble, any row again after 8 steps at the earliest"""
    last = {}
    for t, r in enumerate(rows):
        if r in last:
            d = t - last[r]
            same_or_next_nibble = t // 4 - last[r] // 4 <= 1
            if same_or_next_nibble or d < 8:
                return t
        last[r] = t
    return None


def test_order0_rows_of_a_nibble_are_distinct_and_come_back_two_nibbles_later_at_the_earliest():
    checked = 0
    for name, data in INPUTS.items():
        for bs in BLOCK_SIZES:
            for blk in mr.blocks_of(data, bs)[:70]:
                rows = row_log(blk, mr.ORDER0)
                for i in range(0, len(rows), 4):
                    assert len(set(rows[i:i + 4])) == 4, (name, bs, i)
                    assert not set(rows[i:i + 4]) & set(rows[i + 4:i + 8]), (name, bs, i)
                assert first_violation(rows) is None, (name, bs)
                # the first nibble of a byte stays inside rows 1..15, the second inside 16..255
                assert all((1 <= r <= 15) if (t & 7) < 4 else (16 <= r <= 255) for t, r in enumerate(rows)), (name, bs)
                checked += 1
    assert checked > 300


def test_the_15_nodes_of_a_nibbles_tree_have_15_rows():
    """node (k, x) of the tree of a nibble that starts at partial byte c0 predicts with row (c0 << k) | x: for each of the 17 starts
    (c0 = 1: a byte's first nibble; 16..31: its second) 15 different rows, and no row of a first nibble's tree in a second nibble's"""
    def tree(c0):
        return [(c0 << k) | x for k in range(4) for x in range(1 << k)]
    first = set(tree(1))
    assert len(first) == 15 and first == set(range(1, 16))
    second = set()
    for c0 in range(16, 32):
        t = tree(c0)
        assert len(set(t)) == 15 and not set(t) & first and not set(t) & second
        second |= set(t)
    assert second == set(range(16, 256))


def test_one_weight_set_fails_the_same_check_at_the_first_step():
    for name, data in INPUTS.items():
        rows = row_log(mr.blocks_of(data, 512)[0], mr.ONE)
        assert set(rows) == {0}
        assert first_violation(rows) == 1, name   # step 1 reads what step 0 trained: W3_MIX_ONE stays on the lane kernels


def test_the_log_is_the_mixers_own():
    """the rows a real run of the step logs (two different leaf streams, rate 4) are those of the constant stand-ins"""
    blk = mr.DIRECTED["ramp"]
    log = RowLog()
    n = 8 * len(blk)
    mr.mix([[40000 + (t % 7) for t in range(n)], [9000 + (t % 11) for t in range(n)]], blk, mr.ORDER0, 4, rows=log)
    assert list(log) == row_log(blk, mr.ORDER0)
    assert set(log) == set(range(1, 256))


def test_the_new_exports_are_listed():
    assert "w3_decode_spec_covers" in L.EXPORTS and "w3_last_decode_path" in L.EXPORTS
