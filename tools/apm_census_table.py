"""Prints, as Markdown tables, how often each input of tests/apm_census.py reaches each state of its census, per stage form (the tables
of profiles/apm_census/README.md), and, with --suite, what the inputs of tests/test_gpu_cm.py reached of them before (the main
input of test_cm_models_encode_decode in its 8 KiB blocks and the 64 KiB zero and FF blocks of test_cm_edge_blocks, under the APM
models of that file whose leaves are Counters).  CPU only:  python tools/apm_census_table.py [--suite]"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import apm_census as ac  # noqa: E402

O012 = [ac.O0, ac.O1, ("on", 27, 3)]
# tests/test_gpu_cm.py pair(): the APM models over Counter leaves (name, leaves, stages)
SUITE_MODELS = [("apm0_order0", [ac.O0], [(0, 7)]), ("apm1_order0_r3", [ac.O0], [(1, 3)]), ("apm_rate15", [ac.O1], [(0, 15)]),
                ("apm_rate1", [ac.O1], [(0, 1)]), ("o012_apm", O012, [(0, 7)]), ("apm_chain4", [ac.O0], [(0, 7), (1, 6), (0, 5), (1, 4)])]


def suite_reach():
    """-> (form -> Counter over the main input, form -> Counter over the two 64 KiB edge blocks (o012_apm alone, as the test runs it))"""
    from tests.synth import lcg_text, markov_text, mixed_bytes
    data = markov_text(30000, seed=41) + lcg_text(6000, seed=4) + bytes(700) + mixed_bytes(5000, seed=6)

    def add(into, blk, leaves, stages):
        outs, sk, _ = ac.chain(blk, leaves, stages, engine="schedule")
        outs2, tk, _ = ac.chain(blk, leaves, stages)
        assert outs == outs2
        for k in range(len(stages)):
            form = ac.form_of(stages, k, len(leaves))
            for per_step in (sk[k], tk[k]):
                for names in per_step:
                    for x in names:
                        if x.startswith("mix."):
                            if per_step is sk[k] and k == 0 and stages[0][0] == ac.ORDER0 and len(leaves) > 1:
                                into["mix.L%d" % len(leaves)][x] += 1
                        else:
                            into[form][x] += 1

    main, edge = collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
    for _, leaves, stages in SUITE_MODELS:
        for o in range(0, len(data), 8192):
            add(main, data[o:o + 8192], leaves, stages)
    for blk in (bytes(65536), b"\xff" * 65536):
        add(edge, blk, O012, [(0, 7)])
    return main, edge


def main():
    names = list(ac.INPUTS)
    suite = "--suite" in sys.argv
    print("Inputs (column: name, bytes, leaves, stages as (context kind, rate)):\n")
    for k, name in enumerate(names):
        data, leaves, stages = ac.block(name)
        print("- %d: `%s`, %d bytes, %d leaves, %s" % (k, name, len(data), len(leaves), " ".join("(ORDER%d, %d)" % s for s in stages)))
    if suite:
        smain, sedge = suite_reach()
    for form, required in ac.REQUIRED.items():
        print("\n### `%s`\n" % form)
        cols = [n for n in names if ac.reached(n).get(form)]
        head = ["state"] + [str(names.index(n)) for n in cols] + (["suite main", "suite 64 KiB"] if suite else [])
        print("| " + " | ".join(head) + " |")
        print("|---|" + "---:|" * (len(head) - 1))
        extra = ["out.low_clamp"] if form.endswith(".first") else []
        for state in required + extra:
            row = [str(ac.reached(n)[form][state] or "") for n in cols]
            if suite:
                row += [str(smain[form][state] or ""), str(sedge[form][state] or "")]
            print("| `%s` | " % state + " | ".join(row) + " |")
    print("\nThe launch shapes of k_apm0 (input, block length, blocks):\n")
    for name, length, nblocks in ac.SHAPES:
        print("- `%s`, %d, %d: %s" % (name, length, nblocks, " ".join("`%s`" % k for k in ac.shape_kinds(length, nblocks))))
    print("\nStates that no block of 8 KiB reaches:\n")
    for state, (why, covered_by) in ac.UNREACHABLE_SMALL.items():
        print("- `%s`: %s.  %s." % (state, why, covered_by[0].upper() + covered_by[1:]))


if __name__ == "__main__":
    main()
