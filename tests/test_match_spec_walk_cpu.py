"""The sixteen-lane row's schedule for the match-model leaf (tests/match_spec_ref.py, the restatement of k_decode_spec<.., MATCH>) against
the leaf's definition (tests/match_ref.py): equal streams on every directed input and every small block size, every load of decoded
bytes inside [0, known), every mutant caught, and every single-leaf case of the GPU test proven able to catch what it is there for."""
import pytest

from tests import match_ref as mt
from tests import match_spec_ref as ms


@pytest.mark.parametrize("cfg", mt.CONFIGS)
@pytest.mark.parametrize("name", sorted(mt.DIRECTED))
def test_the_rows_stream_equals_the_definitions(name, cfg):
    m, L = cfg
    x = mt.DIRECTED[name]
    loads = []
    assert ms.row_leaf_stream(x, m, L, loads=loads) == mt.leaf_stream(x, m, L)
    assert all(0 <= p < known for p, known in loads)


@pytest.mark.parametrize("cfg", mt.CONFIGS)
def test_blocks_of_1_to_17_bytes(cfg):
    m, L = cfg
    for src in ("zeros", "pairs", "period_7", "phrases"):
        for n in range(1, 18):
            x = mt.DIRECTED[src][:n]
            loads = []
            assert ms.row_leaf_stream(x, m, L, loads=loads) == mt.leaf_stream(x, m, L), (src, n)
            assert all(0 <= p < known for p, known in loads), (src, n)


def test_every_mutant_is_caught_by_some_directed_input():
    caught = set()
    for name in sorted(mt.DIRECTED):
        caught |= ms.caught_by(mt.DIRECTED[name][:600], 2, 8)
    assert caught == set(ms.MUTANTS)


@pytest.mark.parametrize("name", sorted(ms.GPU_LEAF_CASES))
def test_a_gpu_case_catches_what_it_is_there_for(name):
    """(the mutants a case is meant to catch change its leaf stream; a case blind to all of them would prove nothing on the device)"""
    x, (m, L), meant = ms.GPU_LEAF_CASES[name]
    got = ms.caught_by(x, m, L, sorted(meant))
    assert meant and meant <= got, (sorted(meant - got), sorted(got))
