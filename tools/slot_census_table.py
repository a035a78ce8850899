"""Prints, as a Markdown table, how often each small input of tests/slot_census.py reaches each kind of its census (the table of
profiles/slot_cells/README.md), and what the 65-block layouts reach.  CPU only:  python tools/slot_census_table.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import slot_census as sc  # noqa: E402


def main():
    names = list(sc.SMALL_INPUTS)
    print("Inputs (column: name, bytes, leaf):\n")
    for k, name in enumerate(names):
        data, order, log_cells = sc.block(name)
        print("- %d: `%s`, %d bytes, `SlotModel(%d, %d)`" % (k, name, len(data), order, log_cells))
    print("\n| kind | " + " | ".join(str(k) for k in range(len(names))) + " |")
    print("|---|" + "---:|" * len(names))
    for kind in sc.CELL_KINDS + sc.PIPELINE_KINDS + sc.REPLAY_KINDS + list(sc.UNREACHABLE):
        print("| `%s` | " % kind + " | ".join(str(sc.block_kinds(n)[kind] or "") for n in names) + " |")
    print("\nThe 65-block layouts (64 blocks of 512 bytes and one of 77):\n")
    print("| kind | " + " | ".join("`%s`" % n for n in sc.PIPELINE_INPUTS) + " |")
    print("|---|" + "---:|" * len(sc.PIPELINE_INPUTS))
    lay = {n: sc.kinds(sc.layout_of(n), sc.block(n)[1], sc.block(n)[2], 65, 512) for n in sc.PIPELINE_INPUTS}
    for kind in sc.LAYOUT_KINDS:
        print("| `%s` | " % kind + " | ".join(str(lay[n][kind] or "") for n in sc.PIPELINE_INPUTS) + " |")


if __name__ == "__main__":
    main()
