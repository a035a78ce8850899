"""CPU restatement of the Counter-table leaves k_predict_wave runs (csrc/w3_predict_wave.h), for the tests of a wavefront that walks
several blocks over ONE table (tests/test_match_tags_cpu.py, tests/test_gpu_match_tags.py): the context of every step, and the leaf's
stream over a table that is fresh — what the kernel must give, and what the oracle gives — or carried over from the block before, what a
kernel without its per-block zeroing would give.  Leaves are mixer_ref's descriptions: ("on", bits, align), ("ac", bits, align, max_bits)."""
from tests import mixer_ref as mr
from tests.match_ref import Counter, _lcg

BLOCK = 64
# one leaf of each form the kernel has at this block size (table_form): direct-indexed and exact map, raw history and keyed
LEAVES = {"direct_raw": ("on", 10, 2), "map_raw": ("on", 20, 3), "map_keyed": ("ac", 20, 3, 17), "direct_keyed": ("ac", 10, 2, 8)}


def table_form(leaf, block_size):
    """(a LEAF_WAVE leaf?, exact map?, keyed?) by leaf_class (csrc/w3_twophase.h) and counter_table (csrc/w3_tables_plan.h)"""
    bits, align, keyed = leaf[1], leaf[2], leaf[0] == "ac"
    H = bits - 3
    wave = align != 3 or bits < 3 or (H > 8 and (keyed or H not in (16, 24)))
    slots = 1024
    while slots < 16 * block_size:
        slots *= 2
    return wave, bits >= 32 or (4 << bits) > 8 * slots, keyed


def contexts(orc, leaf, block):
    """the Counter index of every step: ((history & (2^(bits - align) - 1)) << align) | (step & (2^align - 1)), the history being the
    block's bits so far (raw) or ACHistory::hash() of them (keyed, whose first step has context 0)"""
    x = bytes(block)
    bits, align = leaf[1], leaf[2]
    hmask, amask = (1 << (bits - align)) - 1, (1 << align) - 1
    hist = orc.ACHistory(leaf[3], orc.StationaryModel.for_book1()) if leaf[0] == "ac" else None
    out, raw = [], 0
    for t in range(8 * len(x)):
        if hist is None:
            out.append(((raw & hmask) << align) | (t & amask))
        else:
            out.append(0 if t == 0 else ((hist.hash() & hmask) << align) | (t & amask))
        bit = (x[t >> 3] >> (7 - (t & 7))) & 1
        raw = (raw << 1) | bit
        if hist is not None:
            hist.update(bit)
    return out


def stream(orc, leaf, block, table=None):
    """-> (the leaf's probabilities of the block, the table afterwards); table: the Counters the block starts with (default: none)"""
    x = bytes(block)
    tbl = {} if table is None else {k: _copy(c) for k, c in table.items()}
    out = []
    for t, ctx in enumerate(contexts(orc, leaf, x)):
        c = tbl.get(ctx)
        if c is None:
            c = tbl[ctx] = Counter()
        out.append(c.p())
        c.update((x[t >> 3] >> (7 - (t & 7))) & 1)
    return out, tbl


def _copy(c):
    d = Counter()
    d.c0, d.c1 = c.c0, c.c1
    return d


def oracle_blocks(orc, leaf, data, block_size):
    out = []
    for blk in mr.blocks_of(data, block_size):
        out += orc.predict_all(mr.orc_leaf(orc, leaf), bytes(blk)).tolist()
    return out


def inputs():
    """40 equal blocks of 64 B plus a ragged tail, and the same with alternating blocks"""
    a, b = _lcg(BLOCK, 4, 21), _lcg(BLOCK, 4, 22)
    return {"equal": a * 40 + a[:23], "alternating": (a + b) * 20 + a[:23]}
