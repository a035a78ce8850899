"""The sixteen-lane decoder with a match-model leaf among its leaves (k_decode_spec<.., MATCH>, csrc/w3_decode_spec.h; the row's
byte-boundary work: csrc/w3_match_spec_plan.h) behind W3_OPT_VARIANT bit 4096 (decode_match_spec).  Every stream comes from
tests/match_ref.py, the CPU restatement, never from the device's encode (but for the round trip).  With the bit the decode returns the
data on W3_PATH_SPEC; without it, in the same test, on W3_PATH_GENERIC.  Blocks are at most 4 KiB.  What each single-leaf case is there
for, and that it can catch it: tests/match_spec_ref.py, tests/test_match_spec_walk_cpu.py."""
import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests import apm_census as ac
from tests import match_ref as mt
from tests import match_spec_ref as ms
from tests import test_gpu_match as gm   # the whole-model cases and their reference streams, computed once for both files
from weath3rb0i_amd import _lib as L

pytestmark = pytest.mark.gpu
BIT = ("decode_match_spec",)
A0, A1 = (ac.ORDER0, 7), (ac.ORDER1, 6)
TEXT = gm.TEXT
D = mt.DIRECTED

# ---- single leaf: name -> (data, block size, (m, L)) ----------------------------------------------------------------------------------------
# (a) every directed input as one block under the three configurations, `bytes` at L = 20 too (zeros, ones_short: the candidate is the
# byte just stored; period_7, period_64: a candidate a few bytes / a round back; mismatch_bits: the key dies at each of the 8 bit positions)
LEAF_CASES = {nm: (x, 4096, cfg) for nm, (x, cfg, _) in ms.GPU_LEAF_CASES.items()}
# (b) block sizes 1, 3, 7, 8, 9, 63, 65, 200, 4096 with a ragged last block (a block of 1 has none), 1, 2, 3, 4, 5, 9 and 65 blocks: a
# wavefront holds four rows, so the counts that are no multiple of 4 leave idle rows and rows of one wavefront differ in length
SIZE_CASES = {
    "bytes_65_blocks_of_1": (D["bytes"][:65], 1, (2, 8)),
    "pairs_5_blocks_of_3": (D["pairs"][:3 * 4 + 2], 3, (2, 8)),
    "pairs_65_blocks_of_7": (D["pairs"][:7 * 64 + 3], 7, (2, 8)),
    "pairs_2_blocks_of_8": (D["pairs"][100:100 + 8 + 5], 8, (3, 12)),
    "zeros_3_blocks_of_9": (bytes(9 * 2 + 4), 9, (2, 8)),
    "text_4_blocks_of_63": (TEXT[:63 * 3 + 10], 63, (4, 16)),
    "nibbles_9_blocks_of_65": (D["nibbles"][:65 * 8 + 64], 65, (2, 8)),
    "bytes_5_blocks_of_200": (D["bytes"][:200 * 4 + 77], 200, (3, 12)),
    "text_ragged_4096": (TEXT[:4096 + 1000], 4096, (3, 12)),
    "text_1_short_block": (TEXT[:150], 200, (4, 16)),
}
assert {c[1] for c in SIZE_CASES.values()} >= {1, 3, 7, 8, 9, 63, 65, 200, 4096}
assert {-(-len(c[0]) // c[1]) for c in SIZE_CASES.values()} == {1, 2, 3, 4, 5, 9, 65}
assert all(c[1] == 1 or len(c[0]) % c[1] for c in SIZE_CASES.values())
LEAF_CASES.update(SIZE_CASES)
assert max(c[1] for c in LEAF_CASES.values()) <= 4096

# ---- whole models: test_gpu_match's five, plus the tree with the leaf first and last ------------------------------------------------------
MODEL_CASES = dict(gm.MODEL_CASES)
MODEL_CASES.update({
    "tree_match_o0_o1": ((("match", 2, 8), ("o0",), ("o1",)), "tree", (), TEXT[300:300 + 2 * 900 + 50], 900,
                         lambda: w3.BestOfTwoModel(w3.BestOfTwoModel(w3.MatchModel(2, 8), w3.Order0()), w3.Order1())),
    "tree_o0_o1_match": ((("o0",), ("o1",), ("match", 4, 16)), "tree", (), TEXT[2000:2000 + 2 * 900 + 50], 900,
                         lambda: w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.MatchModel(4, 16))),
})
assert set(MODEL_CASES) >= {"order012_match_mix", "tree_o0_match_o1", "leaf_apm01", "full_cm_match_mix_8", "match_mix_65_blocks_of_9"}
assert MODEL_CASES["full_cm_match_mix_8"][0] == mt.full_cm_leaves(8) and MODEL_CASES["full_cm_match_mix_8"][2] == (A0, A1)
assert MODEL_CASES["leaf_apm01"][2] == (A0, A1) and MODEL_CASES["match_mix_65_blocks_of_9"][2] == (A0,)
assert -(-len(MODEL_CASES["match_mix_65_blocks_of_9"][3]) // 9) == 65

# (variant names, W3_OPT_TUNE bits) -> the family: every table format keeps the sixteen-lane decoder, decode_lane and the two-bit groups do not
FORMS = [(BIT, 0, L.W3_PATH_SPEC), (BIT, 131072, L.W3_PATH_SPEC), (BIT, 262144, L.W3_PATH_SPEC), (BIT, 262144 | 524288, L.W3_PATH_SPEC),
         (BIT, 524288, L.W3_PATH_SPEC), (BIT + ("decode_lane",), 0, L.W3_PATH_GENERIC), (BIT, 16384, L.W3_PATH_GENERIC), ((), 0, L.W3_PATH_GENERIC)]

_REF = {}


def leaf_ref(oracle, name):
    if name not in _REF:
        data, bs, (m, Ls) = LEAF_CASES[name]
        comp, lens, _ = mt.encode_blocks(oracle, (("match", m, Ls),), data, bs, "leaf")
        _REF[name] = (np.frombuffer(comp, dtype=np.uint8), np.array(lens, dtype=np.uint32))
    return _REF[name]


def model_ref(oracle, name):
    if name in gm.MODEL_CASES:
        want, wlens, _ = gm.ref(oracle, name)
    else:
        if name not in _REF:
            leaves, combine, stages, data, bs, _ = MODEL_CASES[name]
            _REF[name] = mt.encode_blocks(oracle, leaves, data, bs, combine, stages=stages)
        want, wlens, _ = _REF[name]
    return np.frombuffer(want, dtype=np.uint8), np.array(wlens, dtype=np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def both_families(ctx, model, comp, lens, bs, data):
    """under the bit: W3_PATH_SPEC; without it: W3_PATH_GENERIC; the data both times"""
    try:
        ctx.set_variant(*BIT)
        back = ctx.decode_blocks(model(), comp, lens, bs, len(data))
        assert ctx.last_decode_path() == L.W3_PATH_SPEC
        assert back.tobytes() == data, "sixteen lanes per block"
        ctx.set_variant()
        back = ctx.decode_blocks(model(), comp, lens, bs, len(data))
        assert ctx.last_decode_path() == L.W3_PATH_GENERIC
        assert back.tobytes() == data, "lane per block"
    finally:
        ctx.set_variant()


@pytest.mark.parametrize("name", sorted(LEAF_CASES))
def test_the_single_leaf(ctx, oracle, name):
    data, bs, (m, Ls) = LEAF_CASES[name]
    comp, lens = leaf_ref(oracle, name)
    both_families(ctx, lambda: w3.MatchModel(m, Ls), comp, lens, bs, data)


@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_whole_models(ctx, oracle, name):
    _, _, _, data, bs, model = MODEL_CASES[name]
    comp, lens = model_ref(oracle, name)
    assert w3.Context.decode_spec_covers(model(), variant=BIT) and not w3.Context.decode_spec_covers(model())
    both_families(ctx, model, comp, lens, bs, data)


@pytest.mark.parametrize("name", ["order012_match_mix", "full_cm_match_mix_8"])
def test_every_table_format(ctx, oracle, name):
    _, _, _, data, bs, model = MODEL_CASES[name]
    comp, lens = model_ref(oracle, name)
    try:
        for variant, tune, path in FORMS:
            ctx.set_variant(*variant)
            ctx.set_tune(tune)
            back = ctx.decode_blocks(model(), comp, lens, bs, len(data))
            assert back.tobytes() == data, (variant, tune)
            assert ctx.last_decode_path() == path, (variant, tune)
    finally:
        ctx.set_variant()
        ctx.set_tune(0)


@pytest.mark.parametrize("name", ["order012_match_mix", "tree_o0_match_o1"])
def test_ranges_and_checked_decode(ctx, oracle, name):
    import torch
    _, _, _, data, bs, model = MODEL_CASES[name]
    comp, lens = model_ref(oracle, name)
    n = len(data)
    # a range ending mid-block, one byte at offset 0 (every later job then has an odd destination offset), a range crossing a block
    # boundary, the ragged tail
    ranges = [(100, 901), (0, 1), (bs - 6, 21), (2 * bs + 40, n - 2 * bs - 40)]
    assert 2 * bs < n < 3 * bs
    ranges.append((3, 5))
    assert [sum(ln for _, ln in ranges[:k]) % 2 for k in (1, 3)] == [1, 1]   # odd destination offsets
    want = b"".join(data[o:o + ln] for o, ln in ranges)
    try:
        ctx.set_variant(*BIT)
        assert ctx.decode_ranges(model(), comp, lens, bs, n, ranges).tobytes() == want
        assert ctx.last_decode_path() == L.W3_PATH_SPEC
        d_comp, d_lens = torch.from_numpy(comp.copy()).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
        d_out = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
        assert ctx.decode_ranges_device(model(), d_comp, d_lens, bs, n, ranges, d_out) == len(want)
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == want
        assert ctx.last_decode_path() == L.W3_PATH_SPEC
        # the checked forms: the right table passes, one flipped entry names its block
        crc = ctx.crc32_blocks(data, bs)
        assert ctx.decode_blocks(model(), comp, lens, bs, n, crc=crc).tobytes() == data
        assert ctx.last_decode_path() == L.W3_PATH_SPEC
        assert ctx.decode_ranges(model(), comp, lens, bs, n, ranges, crc=crc).tobytes() == want
        bad = crc.copy()
        bad[1] ^= 1
        with pytest.raises(w3.W3Error) as e:
            ctx.decode_blocks(model(), comp, lens, bs, n, crc=bad)
        assert e.value.code == L.W3_E_CORRUPT and e.value.bad_block == 1
        assert ctx.last_decode_path() == L.W3_PATH_SPEC
        ctx.set_variant()
        assert ctx.decode_ranges(model(), comp, lens, bs, n, ranges).tobytes() == want
        assert ctx.last_decode_path() == L.W3_PATH_GENERIC
    finally:
        ctx.set_variant()


@pytest.mark.parametrize("name", ["match_mix_65_blocks_of_9", "full_cm_match_mix_8"])
def test_device_round_trip(ctx, oracle, name):
    _, _, _, data, bs, model = MODEL_CASES[name]
    ctx.set_path("twophase")
    try:
        out, lens = ctx.encode_blocks(model(), data, bs)
    finally:
        ctx.set_path("auto")
    comp, wlens = model_ref(oracle, name)
    assert lens.tolist() == wlens.tolist() and out.tobytes() == comp.tobytes()
    try:
        ctx.set_variant(*BIT)
        assert ctx.decode_blocks(model(), out, lens, bs, len(data)).tobytes() == data
        assert ctx.last_decode_path() == L.W3_PATH_SPEC
    finally:
        ctx.set_variant()


def test_a_model_without_the_leaf_on_the_same_context(ctx, oracle):
    """decoded before and after a match model under the bit, and under the bit itself: the same bytes on the sixteen-lane decoder"""
    data, bs = TEXT[:2 * 1500 + 77], 1500
    plain = w3.order012_mix
    out, lens = ctx.encode_blocks(plain(), data, bs)
    name = "order012_match_mix"
    _, _, _, mdata, mbs, model = MODEL_CASES[name]
    comp, mlens = model_ref(oracle, name)
    try:
        for variant in ((), BIT, ()):
            ctx.set_variant(*variant)
            assert ctx.decode_blocks(plain(), out, lens, bs, len(data)).tobytes() == data
            assert ctx.last_decode_path() == L.W3_PATH_SPEC
            assert ctx.decode_blocks(model(), comp, mlens, mbs, len(mdata)).tobytes() == mdata
            assert ctx.last_decode_path() == (L.W3_PATH_SPEC if variant else L.W3_PATH_GENERIC)
    finally:
        ctx.set_variant()
