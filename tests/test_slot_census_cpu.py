"""The model and the inputs of tests/test_gpu_slot_cells.py (tests/slot_census.py) checked on the CPU alone.  The Python model of the
slot-state leaf predicts what the oracle predicts, step for step; every named kind of Cell state, of k_slot's pipeline and of the
sorted replay is reached by at least one committed input, and no input reaches a kind the census proves unreachable; for every CELL
kind a model that is wrong in that kind alone predicts differently on an input that reaches it, so a kernel wrong in the same way
cannot pass the GPU run.  The inputs are pinned by their sha256, so that these conditions and the GPU run speak of the same bytes.
Run with -s for the table of which input reaches which kind."""
import collections
import hashlib

import numpy as np
import pytest

from tests import slot_census as sc
from tests.synth import lcg_text, markov_text, mixed_bytes

NAMES = list(sc.SMALL_INPUTS)
SHA256 = {
    "alphabet12_cells4": "48d4157354dd1edf343dc72d29ddb8ee5dde77f93d9a1cee9c8825ae8b4a31f8",
    "alphabet12_cells4_b": "381abb79e3fb3fc5ff9fbc7a9a4dcfdd7c4d026e2ed0307ded51f439d6f2dbd9",
    "runs_shared_cell": "3ebcb790f7e45a8fac86502ad26d1c599dd7ae37ea116a00715cd09ad26e2d89",
    "runs_shared_cell_b": "7ab8a3aebabc1a6af7d3843c4ff623ebd08c527a5f37e1ad500acdf0dd52c284",
    "tag0": "b17339c0eecbbe46288a72431be1b569a258c49cd8455fef23f7779b58461aa3",
    "tag0_b": "6f555ea15273fa7926f346ff8d47f729f581e46c5be121bc8be356af388dc39e",
    "tag0_entrant_tie": "53a77479029886f18800a80ae53c938c9660aedc121b0757323580ae9c4d4c63",
    "random_cells64": "15db6debab68b209eacf0078673cbc7039382dd2997e341f951d0f0175a4d899",
    "random_cells128": "7b4ea2f68ff77d55e9fa0396d0452e58dbfebb2265329e0f69a61e0953a35b33",
    "alphabet40_cells4096": "a8298155c35c722f2568df9db814f7170e45e465d9eaad613110ced393860c4b",
    "alphabet8_cells16": "42837f7408027f573d75cbbe82a73ba3904cfe6a3b700e443bb909ffc203c48b",
    "alphabet5_cells2": "db0c42ba3fcf1e102ca9e612d1647499631fcc614072d8922a2c0f29c3a9cd36",
    "tile_2046": "6c7b00c40d1fd805633206b6263ff67bcd339f7f59060d1660fa7ea0a404c901",
    "tile_2048": "6b3b185f8d205a1d539201e97ec2d36b86787de7d55106bfd6b370fdb236a433",
    "tile_2050": "9767d6f70117483f372e3bec35a74161a621effca73e5e248eb8d2c90ea0ace2",
    "zeros": "d13d4a8b3b8add19b5970157f09d00c12cbda4fed4d74d8493156523f7069b66",
    "ff": "5263250339d3961c91f0bb1150e95ff862f8cd6a4ca873bc8d274dbe86fd6ce7",
    "one_cell": "638d8f43c659418f592a008776d3982998183b19317d037920fd392dd7a715bc",
    "block_of_1": "bbeebd879e1dff6918546dc0c179fdde505f2a21591c9a9c96e36b054ec5af83",
    "block_of_2": "274834e8b3d6a1191aef6436a1d7e8e091370721333f6c6e3658225bc67e0db0",
    "block_of_3": "4ed7f69b3e06570882990f64bf6065d83157635868dab93f0cd7c9ed12da3845",
}
REQUIRED = sc.CELL_KINDS + sc.PIPELINE_KINDS + sc.REPLAY_KINDS
# the slot shapes of tests/test_gpu_cm.py, and its main input
SUITE_SHAPES = [(0, 4), (1, 10), (2, 12), (3, 1), (7, 14), (2, 13)]


def suite_input():
    return markov_text(30000, seed=41) + lcg_text(6000, seed=4) + bytes(700) + mixed_bytes(5000, seed=6)


def reachers():
    """kind -> [(input, count)]"""
    out = collections.defaultdict(list)
    for name in NAMES:
        for kind, count in sc.block_kinds(name).items():
            out[kind].append((name, count))
    return out


def test_the_table_and_the_hash_are_the_oracles(oracle):
    t = oracle.state_table()
    assert t[:, 0].tolist() == sc.PROB and t[:, 1].tolist() == sc.NEXT0 and t[:, 2].tolist() == sc.NEXT1
    assert [oracle.st_conf(s) for s in range(sc.ST_SIZE)] == sc.CONF
    assert sc.NEXT0[sc.PIN0] == sc.PIN0 and sc.NEXT1[sc.PIN1] == sc.PIN1 and max(sc.CONF) == 45
    assert [s for s in range(sc.ST_SIZE) if sc.NEXT0[s] == s or sc.NEXT1[s] == s] == [sc.PIN0, sc.PIN1]
    rng = np.random.default_rng(5)
    for order in range(8):
        hist = rng.integers(0, 2**63, 40, dtype=np.uint64)
        for marker in (0, 0x10, 0x17, 0x1f):
            got = sc.context_hash(order, hist, np.full(40, marker, dtype=np.uint64))
            assert got.tolist() == [oracle.slot_hash(order, int(v), marker != 0, marker & 15) for v in hist], (order, marker)


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_pinned(name):
    data, order, log_cells = sc.block(name)
    assert 0 < len(data) <= 4096
    assert hashlib.sha256(data).hexdigest() == SHA256[name], name


@pytest.mark.parametrize("name", NAMES)
def test_model_predicts_what_the_oracle_predicts(oracle, name):
    data, order, log_cells = sc.block(name)
    got = np.array([x for e in sc.block_events(name) for x in e.p], dtype=np.uint16)
    want = oracle.predict_all(oracle.SlotModel(order, log_cells), data)
    bad = np.flatnonzero(got != want)
    assert not len(bad), sc.describe(data, order, log_cells, int(bad[0]))


@pytest.mark.parametrize("shape", SUITE_SHAPES + [(1, 2), (1, 6), (2, 7), (2, 17)])
def test_model_predicts_what_the_oracle_predicts_on_the_suites_input(oracle, shape):
    data = suite_input()
    for blk in [data[o:o + 8192] for o in range(0, len(data), 8192)] + [bytes(3000), b"\xff" * 3000]:
        assert np.array_equal(sc.predict(blk, *shape), oracle.predict_all(oracle.SlotModel(*shape), blk)), shape


def test_every_kind_is_reached_and_no_unreachable_one():
    reach = reachers()
    print()
    for kind in REQUIRED + list(sc.UNREACHABLE):
        print("  %-44s %s" % (kind, " ".join("%s(%d)" % r for r in reach.get(kind, [])) or "-- no input --"))
    assert len(set(REQUIRED)) == len(REQUIRED) and not set(REQUIRED) & set(sc.UNREACHABLE)
    for kind in REQUIRED:
        assert reach.get(kind), "no input reaches %s" % kind
    for kind in sc.UNREACHABLE:
        assert not reach.get(kind), "%s reaches %s, which the census holds to be unreachable: %s" % (reach[kind], kind, sc.UNREACHABLE[kind])


def test_the_inputs_built_for_a_kind_reach_it():
    """what each directed input is there for, by name"""
    def has(name, *kinds):
        for k in kinds:
            assert sc.block_kinds(name)[k] > 0, "%s does not reach %s" % (name, k)

    has("alphabet12_cells4", *sc.PIPELINE_KINDS[:20])       # every pipeline case at both parities, after an update and after an eviction
    has("runs_shared_cell", *[k for k in sc.CELL_KINDS if "conf" in k], "state.pinned_949")
    has("tag0", "tag0.empty_cell", "tag0.slot3_empty_others_owned", "miss.tag0")
    has("tag0_b", "tag0.empty_cell", "tag0.slot3_empty_others_owned")
    has("tag0_entrant_tie", "tag0.empty_cell", "miss.tie.tag0_entrant")
    has("zeros", "state.pinned_949")
    has("ff", "state.pinned_3962")
    has("one_cell", "replay.one_lane_has_all", "replay.one_pass")
    has("random_cells64", "replay.leaf_w1")
    has("random_cells128", "replay.leaf_w2")
    has("alphabet40_cells4096", "replay.leaf_w4", "replay.cells_share_a_bin", "replay.two_passes")
    has("alphabet8_cells16", "replay.fewer_bins_than_lanes")
    for n in (1, 2, 3):
        has("block_of_%d" % n, "pipe.block_of_%d" % n)
    for n in (2046, 2048, 2050):
        has("tile_%d" % n, "replay.tile_%d" % n)


def test_the_layouts_reach_the_lane_kinds():
    reach = collections.Counter()
    for name in sc.PIPELINE_INPUTS:
        data, order, log_cells = sc.block(name)
        layout = sc.layout_of(name)
        assert len(layout) == 64 * 512 + 77
        reach += sc.kinds(layout, order, log_cells, 65, 512)
    for kind in sc.LAYOUT_KINDS:
        assert reach[kind] > 0, kind


def first_differences(name, mutant):
    """-> (the events at which the mutant's predictions differ from the true model's, the first event at which it may decide differently)"""
    data, order, log_cells = sc.block(name)
    truth = sc.block_events(name)
    got = sc.events(data, order, log_cells, mutant)
    diff = [i for i in range(len(truth)) if truth[i].p != got[i].p]
    scope = [i for i, e in enumerate(truth) if sc.MUTANT_SCOPE[mutant] & set(e.kinds)]
    return diff, (scope[0] if scope else len(truth))


@pytest.mark.parametrize("kind", sc.CELL_KINDS)
def test_a_model_wrong_in_one_kind_predicts_differently(kind):
    """Reaching a kind is not enough: what the kernel does there has to show in the output.  For every CELL kind each mutant that is
    wrong in that kind (slot_census.mutants_of: the first decides differently in that kind alone, a second is a slip of wider scope
    that shows there) predicts differently on an input that reaches it, and predicts what the true model predicts up to the first
    event at which it may decide differently."""
    for mutant in sc.mutants_of(kind):
        assert mutant in sc.MUTANTS
        seen = False
        for name, _ in sorted(reachers()[kind], key=lambda r: -r[1]):
            diff, first = first_differences(name, mutant)
            assert not diff or diff[0] >= first, (kind, mutant, name, "wrong before event %d, the first of its kinds" % first)
            if diff:
                seen = True
                break
        assert seen, "%s: the mutant %s predicts what the true model predicts on every input that reaches the kind" % (kind, mutant)


def test_every_mutant_is_killed_in_some_kind():
    assert {m for kind in sc.CELL_KINDS for m in sc.mutants_of(kind)} == set(sc.MUTANTS)
    assert not set(sc.EQUIVALENT_MUTANTS) & set(sc.MUTANTS)


@pytest.mark.parametrize("mutant", ["le_for_lt", "tags_0_to_3"])
def test_the_compare_slips_show_on_the_input_built_for_them(mutant):
    """<= for < and the tags compared 0 .. 3 look like renamings of a Cell's slots and are none (slot_census.EQUIVALENT_MUTANTS):
    this input is there for them.  Neither is wrong before the tag-0 context has taken its slot and tied with a neighbour."""
    diff, first = first_differences("tag0_entrant_tie", mutant)
    truth = sc.block_events("tag0_entrant_tie")
    entered = next(i for i, e in enumerate(truth) if "tag0.empty_cell" in e.kinds)
    tie = next(i for i, e in enumerate(truth) if "miss.tie.tag0_entrant" in e.kinds)
    assert entered < tie and diff and diff[0] >= first and diff[0] > tie, (mutant, diff[:3], first, entered, tie)


@pytest.mark.parametrize("mutant", sc.EQUIVALENT_MUTANTS)
def test_renaming_the_slots_changes_no_prediction(mutant):
    """The candidate order 0, 1, 2, 3 swaps the names 0 and 1 of a Cell's slots and nothing else (slot_census.EQUIVALENT_MUTANTS has
    the argument): no output can tell it from the true model.  Checked on every input here, the one that separates the other two
    compare slips included, and on tag-0 blocks from other seeds."""
    renamed = 0
    for name in NAMES:
        data, order, log_cells = sc.block(name)
        got = sc.events(data, order, log_cells, mutant)
        assert [e.p for e in got] == [e.p for e in sc.block_events(name)], (mutant, name)
        renamed += sum(a.slot != b.slot for a, b in zip(got, sc.block_events(name)))
    assert renamed, "the mutant never chose another slot: the inputs say nothing about it"
    for seed in range(12):
        data = sc.tag0_block(seed, 1, 1 + seed % 2, 2 + seed % 3, 512)
        assert np.array_equal(sc.predict(data, 2, 1, mutant), sc.predict(data, 2, 1)), (mutant, seed)


def test_the_suites_input_reaches_strictly_fewer_kinds():
    """why the directed inputs exist: the main input of tests/test_gpu_cm.py, in its 8 KiB blocks and slot shapes, leaves kinds unreached"""
    data = suite_input()
    have = set()
    for shape in SUITE_SHAPES[:5]:
        for o in range(0, len(data), 8192):
            have |= set(sc.kinds(data[o:o + 8192], *shape))
    missed = [k for k in REQUIRED if k not in have]
    print("\nthe suite's input misses: %s" % " ".join(missed))
    assert missed
    assert "miss.tie.all4.conf20" in missed and "packed.59" in missed and "replay.leaf_w2" in missed


def test_describe_names_the_event():
    data, order, log_cells = sc.block("tag0")
    e = next(i for i, x in enumerate(sc.block_events("tag0")) if "tag0.empty_cell" in x.kinds)
    text = sc.describe(data, order, log_cells, 4 * e + 2)
    assert "event %d " % e in text and "tag0.empty_cell" in text and "tag 0x000 slot 3" in text
