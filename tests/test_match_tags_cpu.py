"""What tests/test_gpu_match_tags.py's inputs are worth, shown on the CPU.  k_match_keys (csrc/w3_match.h) and k_predict_wave
(csrc/w3_predict_wave.h) give a wavefront a private table and walk the blocks with a grid stride; the GPU test caps the grid
(W3_OPT_WAVE_GRID) so that a wavefront takes hundreds of blocks.  tests/match_ref.py's wave_walk restates that walk — rounds of 64
boundaries, tagged entries, the re-zeroing when the tag returns to 1 — and takes mutants, each one behaviour wrong.  For every shape the
GPU test runs: the steered input's phrase A shares no table entry with the other phrases, every mutant that can show at that shape changes
the LEAF's stream of some block, the mutants of the wrap change the blocks at wavefront sequence 255 and 510 and no others, and the states
the bookkeeping exists for are reached.  And the naive inputs — equal or alternating blocks — are shown NOT to see the wrap mutants, which
is why the inputs are steered.  For k_predict_wave: a table carried over from the block before changes the next block's stream, for every
table form the kernel has."""
import collections

import pytest

from tests import match_ref as mt
from tests import mixer_ref as mr
from tests import wave_ref as wr


def _blocks(data, bs):
    return mr.blocks_of(data, bs)


def _changed(data, bs, waves, m, L, mutant, good):
    """the blocks whose leaf stream the mutant changes (keys first: equal keys give equal streams)"""
    bad = mt.wave_walk(data, bs, waves, m, L, mutant)
    out = []
    for b, blk in enumerate(_blocks(data, bs)):
        if bad[b] != good[b] and mt.stream_of_keys(blk, bad[b]) != mt.stream_of_keys(blk, good[b]):
            out.append(b)
    return out


_WALK = {}


def walked(name):
    """(data, the true walk's keys, its census) of a case, computed once"""
    if name not in _WALK:
        nb, bs, waves, tail, m, L = mt.TAG_CASES[name]
        data = mt.tag_case(name)
        st = collections.Counter()
        _WALK[name] = (data, mt.wave_walk(data, bs, waves, m, L, states=st), st)
    return _WALK[name]


@pytest.mark.parametrize("name", sorted(mt.TAG_CASES))
def test_phrase_a_shares_no_table_entry_with_the_other_phrases(name):
    nb, bs, waves, tail, m, L = mt.TAG_CASES[name]
    A, B, C = mt.tag_phrases(bs, m, L)
    assert len({A, B, C}) == 3
    for k in (m, 2 * m):
        ha = {mt.ctx_hash(A, i, k, L) for i in range(k, bs)}
        for other in (B, C):
            assert not ha & {mt.ctx_hash(other, i, k, L) for i in range(k, bs)}, k
    # and the blocks are where tag_blocks says: A at a wavefront's blocks 0, 255, 510, B and C in turn elsewhere
    data = mt.tag_case(name)
    assert len(data) == nb * bs + tail
    for b, blk in enumerate(_blocks(data, bs)):
        seq = b // waves
        want = A if seq % 255 == 0 else B if seq & 1 else C
        assert blk == want[:len(blk)], b


@pytest.mark.parametrize("name", sorted(mt.TAG_CASES))
def test_the_true_walk_equals_every_block_alone(name):
    nb, bs, waves, tail, m, L = mt.TAG_CASES[name]
    data, good, _ = walked(name)
    assert good == [mt.keys(blk, m, L) for blk in _blocks(data, bs)]


def applicable(name):
    nb, bs, waves, tail, m, L = mt.TAG_CASES[name]
    wraps = (nb - 1) // waves >= 255
    mus = ["no_tag_check", "tag_always_one_no_rezero"]
    if wraps:
        mus += list(mt.WRAP_MUTANTS)
    if wraps and bs > 64:   # a round reads no entry of its own block: only a block of several rounds loses anything to a tag of 256
        mus.append("tag_mod_256")
    return mus


@pytest.mark.parametrize("name", sorted(mt.TAG_CASES))
def test_every_mutant_changes_the_leaf_stream(name):
    nb, bs, waves, tail, m, L = mt.TAG_CASES[name]
    data, good, _ = walked(name)
    nblk = len(_blocks(data, bs))
    for mu in applicable(name):
        ch = _changed(data, bs, waves, m, L, mu, good)
        assert ch, mu
        seqs = {b // waves for b in ch}
        if mu in mt.WRAP_MUTANTS:
            want = [b for b in range(nblk) if b // waves in (255, 510)]
            assert ch == want, (mu, ch)
        elif mu == "tag_mod_256":
            assert seqs <= {255, 511}, (mu, sorted(seqs))
        else:   # without the tag check a block meets the entries of the last block of its phrase: all but a phrase's first after a zeroing
            zeroings = ((nblk - 1) // waves) // 255 + 1
            assert len(ch) >= nblk - 3 * waves * zeroings, (mu, len(ch))


def test_the_census_reaches_every_state_of_the_bookkeeping():
    for name in mt.TAG_CASES:
        nb, bs, waves, tail, m, L = mt.TAG_CASES[name]
        st = walked(name)[2]
        assert st["stale_tag_rejected"] >= 1 and st["stale_pos_at_or_past_boundary"] >= 1, name
        if tail:
            assert st["stale_pos_past_short_last_block"] >= 1, name
        if (nb - 1) // waves >= 255:
            assert st["entry_cleared_at_wrap_would_have_hit"] >= 1 and st["long_table_only_stale"] >= 1, name
    assert any(t[3] for t in mt.TAG_CASES.values())


def test_naive_inputs_cannot_see_the_wrap_mutants():
    """why the inputs are steered: with 520 equal or three-way alternating blocks every block overwrites what would have gone stale"""
    P = [mt._phrase(24, 2, s) for s in (1, 2, 3)]
    for data in (P[0] * 520, b"".join(P[b % 3] for b in range(520))):
        good = mt.wave_walk(data, 24, 1, 2, 12)
        for mu in mt.WRAP_MUTANTS:
            assert mt.wave_walk(data, 24, 1, 2, 12, mu) == good, mu
        bad = mt.wave_walk(data, 24, 1, 2, 12, "no_tag_check")
        assert len([b for b in range(520) if bad[b] != good[b]]) >= 510


def test_wavefronts_with_two_blocks_beside_wavefronts_with_one():
    data = mt.two_block_waves()
    good = mt.wave_walk(data, 24, 64, 2, 8)
    assert good == [mt.keys(blk, 2, 8) for blk in _blocks(data, 24)]
    for mu in ("no_tag_check", "tag_always_one_no_rezero"):
        assert _changed(data, 24, 64, 2, 8, mu, good) == list(range(64, 70)), mu   # the six second blocks


def test_the_long_block_uses_the_position_field_above_bit_16():
    x = mt.long_block()
    assert len(x) == 70000 and x[100:140] == x[66000:66040] == x[68500:68540]
    st = collections.Counter()
    good = mt.wave_walk(x, 131072, 1, 4, 20, states=st)
    assert good == [mt.keys(x, 4, 20)]
    assert st["cand_65536_or_more_back"] >= 1 and st["cand_pos_65536_or_more"] >= 1
    assert _changed(x, 131072, 1, 4, 20, "pos_16_bits", good) == [0]


# ---- k_predict_wave: the table of the block before -------------------------------------------------------------------------------------
def test_the_wave_leaves_cover_every_table_form():
    forms = {nm: wr.table_form(lf, wr.BLOCK) for nm, lf in wr.LEAVES.items()}
    assert all(f[0] for f in forms.values())   # every one a leaf of k_predict_wave
    assert {f[1:] for f in forms.values()} == {(False, False), (True, False), (True, True), (False, True)}
    assert forms["direct_raw"][1:] == (False, False) and forms["map_raw"][1:] == (True, False) and forms["map_keyed"][1:] == (True, True)


@pytest.mark.parametrize("leaf", sorted(wr.LEAVES))
@pytest.mark.parametrize("kind", ["equal", "alternating"])
def test_a_table_carried_over_changes_the_next_blocks_stream(oracle, leaf, kind):
    lf = wr.LEAVES[leaf]
    data = wr.inputs()[kind]
    blocks = _blocks(data, wr.BLOCK)
    assert len(blocks) == 41 and len(blocks[-1]) == 23
    # the restatement over a fresh table is the oracle's leaf
    fresh = [wr.stream(oracle, lf, blk) for blk in blocks[:3]]
    for blk, (p, _) in zip(blocks[:3], fresh):
        assert p == oracle.predict_all(mr.orc_leaf(oracle, lf), bytes(blk)).tolist()
    # over the table the block before left, block 1's stream (and the last, short block's) is another
    assert wr.stream(oracle, lf, blocks[1], fresh[0][1])[0] != fresh[1][0]
    tail_fresh = wr.stream(oracle, lf, blocks[-1])[0]
    assert wr.stream(oracle, lf, blocks[-1], wr.stream(oracle, lf, blocks[-2])[1])[0] != tail_fresh
