"""The model and the inputs of tests/test_gpu_apm_states.py (tests/apm_census.py) checked on the CPU alone.  The Python model of an APM
chain predicts what the oracle predicts, stage by stage and step for step, in time order and in k_apm0's / k_apm1's order; every named
state is reached by a committed input for every stage form; the states that a block of 8 KiB cannot reach are listed with the
arithmetic and with the test that does reach them; a model with one behaviour changed predicts differently from the oracle on at
least one input, so a kernel wrong in the same way cannot pass the GPU run.  The inputs are pinned by their sha256, so that these
conditions and the GPU run speak of the same bytes.  Run with -s for which input reaches which state and catches which mutant."""
import collections
import hashlib

import numpy as np
import pytest

from tests import apm_census as ac
from tests.synth import lcg_text, markov_text, mixed_bytes

NAMES = list(ac.INPUTS)
SHA256 = {
    "zeros_bits": "7a244716531720907237fc6bff10ba594897d2a73b92af1b93ef17cfbd833c34",
    "ones_bits": "564f2862e6c39d2177320410d66db89b7cfbce372ce8253081e64fd5441e2afc",
    "runs41": "3ebc90912406b24898f6f6a09bc32d9892c535c01846e9aec5100a2ae14f41c1",
    "marked0": "e80a8b39caf023f7d90f1a6c66e63b1a5a6a170ffde1e9230ed86d34411076eb",
    "marked1": "825b2e6acbfd0f1cb6fb442fe5861f13189510a2494f8f30e9ce50ef9142fb21",
    "ff_decay": "31ba4dad3e4073593f2ec15ddc5955b27b15fe946f04674fc94e0e8aa56e94a3",
    "ramp": "da57be507319dc2343f7beead277aa3eb25a15f05445e8c93fabcb8f0b3f6b01",
    "alphabet4": "33a707985809076c16383950a72b5501db10bee0b366581606e57ff3c2945c1c",
}
_oracle_streams = {}


def oracle_streams(oracle, name):
    """the oracle's stream of every chain prefix of the named input (0 stages = the mixed leaves), made once"""
    if name not in _oracle_streams:
        data, leaves, stages = ac.block(name)
        _oracle_streams[name] = [oracle.predict_all(ac.build(oracle, leaves, stages[:k]), data).tolist() for k in range(len(stages) + 1)]
    return _oracle_streams[name]


def counter_p(n):
    """Counter::p after n visits with bit 0"""
    p = (1 << 17) // (n + 2)
    return (p >> 1) + (p & 1)


def test_the_tables_are_the_oracles(oracle):
    assert [oracle.squash(d) for d in range(-2047, 2048)] == ac.SQUASH
    assert [oracle.stretch(16 * q) for q in range(4096)] == ac.STRETCH
    assert oracle.squash(-5000) == ac.squash(-5000) == ac.SQUASH[0] and oracle.squash(5000) == ac.squash(5000) == ac.SQUASH[-1]
    assert min(ac.STRETCH) == -2047 and max(ac.STRETCH) == 2047
    assert ac.STRETCH[0] == -2047 and ac.STRETCH[1] > -2047, "stretch = -2047 needs p <= 15"
    assert ac.ROW_INIT[16] == 32768 and ac.ROW_INIT[0] == ac.SQUASH[0] and ac.ROW_INIT[32] == ac.SQUASH[-1]


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_pinned(name):
    data, leaves, stages = ac.block(name)
    assert 0 < len(data) <= (8192 if name.startswith(("zeros_bits", "ones_bits")) else 4096)
    assert hashlib.sha256(data).hexdigest() == SHA256[name.split(".")[0]], name
    assert 1 <= len(leaves) <= 8 and 1 <= len(stages) <= 4


@pytest.mark.parametrize("name", NAMES)
def test_model_predicts_what_the_oracle_predicts(oracle, name):
    """every stage's stream, in time order and in the kernels' order (apm_census.block_kinds asserts that the two agree)"""
    got, want = ac.block_streams(name), oracle_streams(oracle, name)
    assert len(got) == len(want)
    for k in range(len(want)):
        bad = [s for s in range(len(want[k])) if got[k][s] != want[k][s]]
        assert not bad, "%d steps differ in the stream of %d stages, the first: got %d, want %d at %s" % (
            len(bad), k, got[k][bad[0]], want[k][bad[0]], ac.describe(name, k - 1, bad[0]) if k else "step %d of the mixed leaves" % bad[0])


def reachers():
    """form -> state -> [(input, count)]"""
    out = collections.defaultdict(lambda: collections.defaultdict(list))
    for name in NAMES:
        for form, states in ac.reached(name).items():
            for state, count in states.items():
                out[form][state].append((name, count))
    return out


def test_every_state_is_reached_for_every_stage_form():
    reach = reachers()
    print()
    for form, required in ac.REQUIRED.items():
        assert len(set(required)) == len(required)
        for state in required:
            print("  %-14s %-52s %s" % (form, state, " ".join("%s(%d)" % r for r in reach[form].get(state, [])) or "-- no input --"))
    for form, required in ac.REQUIRED.items():
        for state in required:
            assert reach[form].get(state), "no input reaches %s in a stage of form %s" % (state, form)


def test_the_forms_cover_the_leaf_counts_and_the_rates():
    first0 = {len(ac.block(n)[1]) for n in NAMES if ac.block(n)[2][0][0] == ac.ORDER0}
    assert set(ac.FIRST_STAGE_LEAF_COUNTS) <= first0, first0
    rates = {r for n in NAMES for _, r in ac.block(n)[2]}
    assert set(ac.RATES) <= rates, rates
    assert any(len(ac.block(n)[2]) <= 2 for n in NAMES) and any(len(ac.block(n)[2]) == 4 for n in NAMES)


def test_the_first_two_stages_reach_every_state_of_a_step():
    """k_decode_spec takes at most two stages: tests/test_gpu_apm_states.py decodes the two-stage prefix of every longer chain with it,
    and those prefixes, with the chains of one and two stages, reach every state of a step's arithmetic and rows but the low clamp
    (UNREACHABLE_SMALL).  The pair and path states belong to k_apm0's and k_apm1's order and mean nothing to a decoder."""
    two_stage = collections.Counter()
    for n in NAMES:
        fs, _ = ac.forms(n)
        for k, per_step in enumerate(ac.block_kinds(n)[:2]):
            two_stage.update((fs[k], x) for names in per_step for x in names)
    for form in ac.FORMS:
        rows = ac.ROW0_KINDS if form.startswith("order0") else ac.ROW1_KINDS
        missed = [s for s in ac.LOOKUP_KINDS + ac.INTERP_KINDS + ac.UPDATE_KINDS + rows if not two_stage[(form, s)]]
        assert not missed, (form, missed)
        assert not two_stage[(form, "out.low_clamp")]


def test_the_inputs_built_for_a_state_reach_it():
    """what each directed input is there for, by name"""
    def has(name, form, *states):
        for s in states:
            assert ac.reached(name)[form][s] > 0, "%s does not reach %s in %s" % (name, s, form)

    has("zeros_bits.o0", "order0.first", "stretch.-2047", "update.arrives_at_0", "update.stays_0", "entry.0.bit0", "entry.0.bit1")
    has("zeros_bits.o0", "order0.later", "out.low_clamp")
    has("zeros_bits.o0", "order1.later", "out.low_clamp", "apm1.fast:out.low_clamp")
    has("zeros_bits.o1", "order1.first", "stretch.-2047", "entry.0.bit1")
    has("ones_bits.o0", "order0.first", "stretch.+2047", "update.stall", "entry.32.bit1", "entry.32.bit0")
    has("ones_bits.o1", "order1.first", "stretch.+2047", "entry.32.bit0")
    has("runs41.o0", "order0.first", "update.leaves_0", "w.2048", "w.0", "pair.different_rows", *ac.FORWARD_KINDS)
    second = ac.reached("runs41.o0")["order0.later"]
    assert all(second["entry.%d.bit0" % e] + second["entry.%d.bit1" % e] for e in range(33)), "runs41's second stage trains all 33 entries"
    has("marked0", "order1.later", *ac.APM1_CROSS_KINDS)
    has("marked0.first", "order1.first", "apm1.slow:update.arrives_at_0", "apm1.slow:update.stays_0", "apm1.slow:update.leaves_0")
    has("marked1.first", "order1.first", "apm1.slow:update.stall")
    has("ff_decay.o0", "order0.first", *["entry.%d.bit0" % e for e in range(21, 32)])
    has("ff_decay.o1", "order1.first", *["entry.%d.bit0" % e for e in range(21, 32)])
    has("ramp.o0", "order0.first", *ac.ROW0_KINDS)
    has("ramp.o0", "order0.later", *ac.ROW0_KINDS)
    has("ramp.o1", "order1.first", *ac.ROW1_KINDS)
    for n in ("alphabet4.L2", "alphabet4.L3", "alphabet4.L7"):
        has(n, "mix." + n[-2:], *ac.REQUIRED["mix." + n[-2:]])


def test_the_shapes_reach_the_launch_kinds(oracle):
    """k_apm0's launch shapes: every kind is named by a shape, and the schedule model agrees with the oracle on every block of them"""
    seen = collections.Counter()
    for name, length, nblocks in ac.SHAPES:
        seen.update(ac.shape_kinds(length, nblocks))
        data = ac.shape_data(name, length, nblocks)
        _, leaves, stages = ac.block(name)
        assert len(data) == length * nblocks
        for o in range(0, len(data), length):
            got = ac.chain(data[o:o + length], leaves, stages, engine="schedule", with_kinds=False)[0][-1]
            assert got == oracle.predict_all(ac.build(oracle, leaves, stages), data[o:o + length]).tolist(), (name, length, o)
    for kind in ac.SHAPE_KINDS:
        assert seen[kind], kind


# ---- what a block of the census's size cannot reach -------------------------------------------------------------------------------------
def test_the_arithmetic_of_the_unreachable_states():
    assert min(n for n in range(70000) if counter_p(n) == 1) == 43689
    assert min(n for n in range(70000) if counter_p(n) <= 5) == 11914
    assert min(n for n in range(70000) if counter_p(n) <= 15) == 4227        # (stretch = -2047: the one state that needs more than 4 KiB)
    assert all(((p + 2) >> 2 == 1) == (2 <= p <= 5) for p in range(1, 200)), "a second stage sees p = 1 only behind a leaf p <= 5"
    assert (65535 + 3 * 65535 + 2) >> 2 == 65535
    for rate in range(1, 16):
        t = 65535 - ((1 << rate) - 1)
        assert (65535 - t) >> rate == 0 and (65535 - (t - 1)) >> rate == 1
        assert ac.SQUASH[-1] <= 65535 - 1
    reach = reachers()
    assert not reach["order0.first"].get("out.low_clamp") and not reach["order1.first"].get("out.low_clamp")
    for n in NAMES:                              # no second stage clamps either
        kinds = ac.block_kinds(n)
        if len(kinds) > 1:
            assert not any("out.low_clamp" in k for k in kinds[1]), n
    print()
    for state, (why, covered_by) in ac.UNREACHABLE_SMALL.items():
        print("  %s: %s.  %s" % (state, why, covered_by))
    assert sum(c.startswith("UNCOVERED") for _, c in ac.UNREACHABLE_SMALL.values()) == 1


def test_the_64k_zero_block_of_the_suite_reaches_the_first_stage_clamp(oracle):
    """tests/test_gpu_cm.py::test_cm_edge_blocks runs 65,536 zero bytes through o012_apm: the model says that its one stage clamps, and that
    a second stage behind it (full_cm_small_tables has APM(ORDER1, 6) there; whenever Order0 gives p = 1 no other leaf is farther
    from 1/2, so the mix is Order0's) clamps too"""
    data = bytes(65536)
    leaves = [ac.O0, ac.O1, ("on", 27, 3)]
    outs, kinds, _ = ac.chain(data, leaves, [(0, 7), (1, 6)])
    assert outs[1] == oracle.predict_all(ac.build(oracle, leaves, [(0, 7)]), data).tolist()
    first = sum("out.low_clamp" in k for k in kinds[0])
    second = sum("out.low_clamp" in k for k in kinds[1])
    print("\n  steps at the low clamp: %d in the first stage, %d in the second" % (first, second))
    assert first > 0 and second > 0
    assert min(outs[0]) == 1


# ---- would a wrong kernel be noticed? --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ac.ALL_MUTANTS)
def test_a_model_wrong_in_one_behaviour_predicts_differently(oracle, mutant):
    """the model with exactly one behaviour changed (apm_census: STAGE_MUTANTS in the step's arithmetic, SCHED_MUTANTS in k_apm0's and
    k_apm1's pair forwarding and hand-over, APM1_MUTANTS, MIX_MUTANTS) against the oracle, on every census input"""
    caught = []
    for name in NAMES:
        data, leaves, stages = ac.block(name)
        want = oracle_streams(oracle, name)
        got = ac.chain(data, leaves, stages, mutant=mutant, with_kinds=False, truth=want)[0]
        for k in range(len(got)):
            if got[k] != want[k]:
                s = next(i for i in range(len(want[k])) if got[k][i] != want[k][i])
                caught.append("%s (stream of %d stages, step %d)" % (name, k, s))
                break
    print("\n  %s is caught by: %s" % (mutant, "; ".join(caught) or "-- no input --"))
    assert caught, "the mutant %s predicts what the oracle predicts on every census input" % mutant
    # (none of the mutants is a renaming: each is caught, so none needs the argument that it cannot be)


def test_the_mutants_named_by_the_issue_are_all_there():
    assert len(set(ac.ALL_MUTANTS)) == len(ac.ALL_MUTANTS) == 14
    assert set(ac.ALL_MUTANTS) == {
        "update_truncates", "interp_truncates", "tie_to_lower", "no_low_clamp", "init_no_clip", "stale_same_entry", "stale_other_entry",
        "earlier_store_wins", "forward_on_earlier_other", "batch_handover_lost", "order1_c1_is_current", "no_reinit_at_group_change",
        "mix_tie_right", "mix_cross_halves"}


# ---- why the directed inputs exist ----------------------------------------------------------------------------------------------------
def suite_input():
    """the input of tests/test_gpu_cm.py::test_cm_models_encode_decode"""
    return markov_text(30000, seed=41) + lcg_text(6000, seed=4) + bytes(700) + mixed_bytes(5000, seed=6)


def test_the_suites_input_reaches_strictly_fewer_states(oracle):
    """o012_apm, the k_apm0<3> form the bench runs, over the suite's main input in its 8 KiB blocks: the end entries are never trained
    and stretch never reaches an end"""
    data = suite_input()
    leaves = [ac.O0, ac.O1, ("on", 27, 3)]
    have = collections.Counter()
    for o in range(0, len(data), 8192):
        blk = data[o:o + 8192]
        outs, kinds, _ = ac.chain(blk, leaves, [(0, 7)])
        assert outs[1] == oracle.predict_all(ac.build(oracle, leaves, [(0, 7)]), blk).tolist()
        have.update(x for k in kinds[0] for x in k)
    missed = [s for s in ac.LOOKUP_KINDS + ac.INTERP_KINDS + ac.UPDATE_KINDS if not have[s]]
    print("\n  o012_apm over the suite's input misses: %s" % " ".join(missed))
    assert "stretch.-2047" in missed and "stretch.+2047" in missed
    assert {int(s.split(".")[1]) for s in have if s.startswith("entry.")} == set(range(2, 31))


def test_describe_names_the_step():
    kinds = ac.block_kinds("marked0")[3]
    s = next(i for i, k in enumerate(kinds) if "apm1.slow:out.low_clamp" in k)
    text = ac.describe("marked0", 3, s)
    assert "stage 3 (ORDER1, rate 1, order1.later)" in text and "step %d " % s in text and "out.low_clamp" in text and "input p 1," in text
