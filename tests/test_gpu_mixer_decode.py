"""Decode of logistic-mixer specs (W3_NODE_MIX, W3_MIX_ORDER0) by the sixteen-lane decoder (k_decode_spec with its mixer parameter,
csrc/w3_decode_spec.h) against tests/mixer_ref.py, the CPU restatement: the reference's streams must decode to the data in every table
format and on the lane kernels, w3_last_decode_path must name the kernel family that ran, byte ranges and the checked decode take the
same path, and w3_decode_spec_covers answers for the specs on either side of the rule.  Blocks are at most 4 KiB."""
import ctypes as C

import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests import apm_census as ac
from tests import mixer_ref as mr
from tests.synth import lcg_text, markov_text
from weath3rb0i_amd import _lib as L

pytestmark = pytest.mark.gpu

L2 = mr.DIRECTED_LEAVES
L3 = (("o0",), ("o1",), ("on", 27, 3))
L8 = (("o0",), ("o1",), ("on", 27, 3), ("on", 8, 3), ("ac", 11, 3, 8), ("on", 14, 4), ("on", 5, 3), ("on", 22, 2))   # an `ac` leaf, an alignment-2 leaf
L7S = (("o0",), ("o1",), ("on", 27, 3), ("slot", 1, 10), ("slot", 2, 10), ("slot", 3, 10), ("slot", 4, 10))
A0, A1 = (ac.ORDER0, 7), (ac.ORDER1, 6)
TEXT = markov_text(6000, seed=23) + lcg_text(1200, seed=5) + bytes(300) + b"\xff" * 300

# name: (leaves, rate, APM chain, data, block size), selector ORDER0.  Block counts 1, 2, 3, 4, 5, 9, 65 (a wavefront holds four blocks: the
# counts that are no multiple of 4 leave idle rows in the last one); block sizes 1, 7, 9, 512, 4096 (and 300, 2048); ragged last blocks.
DIRECTED_USED = ("zeros_then_ff00", "runs_00_ff", "ramp")
CASES = {
    "n2_r4_zeros_then_ff00_1_block": (L2, 4, (), mr.DIRECTED["zeros_then_ff00"], 4096),
    "n2_r4_runs_00_ff_1_block": (L2, 4, (), mr.DIRECTED["runs_00_ff"], 4096),
    "n2_r4_ramp_1_block": (L2, 4, (), mr.DIRECTED["ramp"], 512),
    "n2_r4_apm1_ramp_ragged": (L2, 4, (A1,), mr.DIRECTED["ramp"] + bytes(range(200)), 512),
    "n2_r4_apm0_zeros_ones": (L2, 4, (A0,), mr.DIRECTED["zeros"][:2048] + mr.DIRECTED["ones"][:2048], 2048),
    "n3_r14_3_blocks_ragged": (L3, 14, (), TEXT[6700:6700 + 2 * 512 + 76], 512),
    "n3_r20_apm1_65_blocks_of_9": (L3, 20, (A1,), TEXT[:9 * 64 + 5], 9),
    "n3_r14_9_blocks_of_1": (L3, 14, (), TEXT[:9], 1),
    "n3_r14_apm0_5_blocks_of_7": (L3, 14, (A0,), TEXT[100:100 + 4 * 7 + 3], 7),
    "n8_r14_apm01_ragged": (L8, 14, (A0, A1), TEXT[:4096 + 1000], 4096),
    "n8_r20_apm0_4_blocks": (L8, 20, (A0,), TEXT[2000:2000 + 4 * 300], 300),
    "n8_r4_65_blocks_of_1": (L8, 4, (), TEXT[300:365], 1),
    "n7_slots_r14_apm01_ragged": (L7S, 14, (A0, A1), TEXT[:4096 + 333], 4096),
    "n7_slots_r4_apm1_9_blocks_of_9": (L7S, 4, (A1,), TEXT[500:500 + 8 * 9 + 2], 9),
    "n7_slots_r20_1_block": (L7S, 20, (), TEXT[6000:6512], 512),
    "n7_slots_r14_apm0_2_blocks": (L7S, 14, (A0,), TEXT[6900:7800], 512),
}
N_BLOCKS = {name: -(-len(c[3]) // c[4]) for name, c in CASES.items()}
assert set(N_BLOCKS.values()) == {1, 2, 3, 4, 5, 9, 65}
assert {c[4] for c in CASES.values()} >= {1, 7, 9, 512, 4096} and max(c[4] for c in CASES.values()) <= 4096
assert {c[1] for c in CASES.values()} == {4, 14, 20} and {c[2] for c in CASES.values()} == {(), (A0,), (A1,), (A0, A1)}

# (variant names, W3_OPT_TUNE bits) -> the kernel family a covered mixer spec decodes on: the table formats forced either way (bits 17 /
# 18) and the general-kernel bit (19) keep the sixteen-lane decoder, decode_lane asks for the lane kernels, and under the two-bit-group
# variant (bit 14), which is not built for the mixer, a mixer spec goes to the lane kernels too
FORMS = [((), 0, L.W3_PATH_SPEC), ((), 131072, L.W3_PATH_SPEC), ((), 262144, L.W3_PATH_SPEC), ((), 262144 | 524288, L.W3_PATH_SPEC),
         ((), 524288, L.W3_PATH_SPEC), (("decode_lane",), 0, L.W3_PATH_GENERIC), ((), 16384, L.W3_PATH_GENERIC)]

_REF = {}


def ref(oracle, name, select=mr.ORDER0):
    """(streams as np.uint8, block lengths as np.uint32) of the case from the CPU restatement, computed once"""
    if (name, select) not in _REF:
        leaves, rate, stages, data, bs = CASES[name]
        comp, lens, _ = mr.encode_blocks(oracle, leaves, data, bs, select, rate, stages)
        _REF[name, select] = (np.frombuffer(comp, dtype=np.uint8), np.array(lens, dtype=np.uint32))
    return _REF[name, select]


def model_of(name, select=mr.ORDER0):
    leaves, rate, stages, _, _ = CASES[name]
    return mr.w3_model(w3, leaves, select, rate, stages)


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def test_no_decode_yet():
    c = w3.Context(0)
    try:
        assert c.last_decode_path() == 0
        assert c.lib.w3_last_decode_path(None) == 0
    finally:
        c.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_streams_decode_in_every_form(ctx, oracle, name):
    _, _, _, data, bs = CASES[name]
    comp, lens = ref(oracle, name)
    assert w3.Context.decode_spec_covers(model_of(name))
    try:
        for variant, tune, path in FORMS:
            ctx.set_variant(*variant)
            ctx.set_tune(tune)
            back = ctx.decode_blocks(model_of(name), comp, lens, bs, len(data))
            assert back.tobytes() == data, (variant, tune)
            assert ctx.last_decode_path() == path, (variant, tune)
    finally:
        ctx.set_variant()
        ctx.set_tune(0)


def test_the_directed_cases_reach_every_clamp_and_every_row(oracle):
    """the claim behind the cases above, checked on the CPU side: the directed inputs they decode reach every state of mr.STATES under
    ORDER0 at rate 4 (the rate and leaves of the n2_r4 cases, each input one whole block there) and every ORDER0 row"""
    states, rows = {}, set()
    for name in DIRECTED_USED:
        whole = [c for c in CASES.values() if c[0] == mr.DIRECTED_LEAVES and c[1] == 4 and c[3] == mr.DIRECTED[name] and c[4] >= len(c[3])]
        assert whole, name
        st, rw = mr.reached(oracle, name, mr.ORDER0, 4)
        for k, v in st.items():
            states[k] = states.get(k, 0) + v
        rows |= rw
    assert all(states.get(k, 0) > 0 for k in mr.STATES), states
    assert rows == set(range(1, 256))


def test_mix_one_stays_on_the_lane_kernels(ctx, oracle):
    name = "n3_r14_apm0_5_blocks_of_7"
    _, _, _, data, bs = CASES[name]
    comp, lens = ref(oracle, name, mr.ONE)
    assert not w3.Context.decode_spec_covers(model_of(name, mr.ONE))
    assert ctx.decode_blocks(model_of(name, mr.ONE), comp, lens, bs, len(data)).tobytes() == data
    assert ctx.last_decode_path() == L.W3_PATH_GENERIC
    # ... and the same leaves under ORDER0 go back to the sixteen-lane decoder on the same context
    comp, lens = ref(oracle, name)
    assert ctx.decode_blocks(model_of(name), comp, lens, bs, len(data)).tobytes() == data
    assert ctx.last_decode_path() == L.W3_PATH_SPEC


@pytest.mark.parametrize("name", ["n7_slots_r14_apm01_ragged", "n8_r14_apm01_ragged"])
def test_ranges_and_checked_decode(ctx, oracle, name):
    import torch
    _, _, _, data, bs = CASES[name]
    comp, lens = ref(oracle, name)
    n = len(data)
    # a range ending mid-block, one byte at offset 0, a range crossing the block boundary, the ragged tail
    ranges = [(100, 1900), (0, 1), (4090, 20), (4200, n - 4200)]
    want = b"".join(data[o:o + ln] for o, ln in ranges)
    model = model_of(name)
    assert ctx.decode_ranges(model, comp, lens, bs, n, ranges).tobytes() == want
    assert ctx.last_decode_path() == L.W3_PATH_SPEC
    ctx.set_variant("decode_lane")
    try:
        assert ctx.decode_ranges(model, comp, lens, bs, n, ranges).tobytes() == want
        assert ctx.last_decode_path() == L.W3_PATH_GENERIC
    finally:
        ctx.set_variant()
    d_comp, d_lens = torch.from_numpy(comp.copy()).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    d_out = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
    assert ctx.decode_ranges_device(model, d_comp, d_lens, bs, n, ranges, d_out) == len(want)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == want
    assert ctx.last_decode_path() == L.W3_PATH_SPEC
    # the checked forms: the right table passes, one flipped entry names its block
    crc = ctx.crc32_blocks(data, bs)
    assert ctx.decode_blocks(model, comp, lens, bs, n, crc=crc).tobytes() == data
    assert ctx.last_decode_path() == L.W3_PATH_SPEC
    assert ctx.decode_ranges(model, comp, lens, bs, n, ranges, crc=crc).tobytes() == want
    bad = crc.copy()
    bad[1] ^= 1
    with pytest.raises(w3.W3Error) as e:
        ctx.decode_blocks(model, comp, lens, bs, n, crc=bad)
    assert e.value.code == L.W3_E_CORRUPT and e.value.bad_block == 1
    assert ctx.last_decode_path() == L.W3_PATH_SPEC


@pytest.mark.parametrize("name", ["n3_r20_apm1_65_blocks_of_9", "n7_slots_r14_apm0_2_blocks"])
def test_device_round_trip(ctx, oracle, name):
    _, _, _, data, bs = CASES[name]
    ctx.set_path("twophase")
    try:
        out, lens = ctx.encode_blocks(model_of(name), data, bs)
    finally:
        ctx.set_path("auto")
    comp, wlens = ref(oracle, name)
    assert lens.tolist() == wlens.tolist() and out.tobytes() == comp.tobytes()
    assert ctx.decode_blocks(model_of(name), out, lens, bs, len(data)).tobytes() == data
    assert ctx.last_decode_path() == L.W3_PATH_SPEC


def test_decode_spec_covers():
    covers = w3.Context.decode_spec_covers
    o012 = w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3))
    for m in (w3.order012_mix(), w3.full_cm_mix(), o012, w3.full_cm(), mr.w3_model(w3, L8, mr.ORDER0, 14, (A0, A1))):
        assert covers(m) is True
    for m in (mr.w3_model(w3, L2, mr.ONE, 14), mr.w3_model(w3, L7S, mr.ONE, 4, (A0,)),             # one weight set: every bit feeds the next
              mr.w3_model(w3, (("o0",), ("on", 32, 1)), mr.ORDER0, 14),                            # a leaf with alignment 1
              w3.LogisticMixer([w3.Order0(), w3.OrderN(32, 1)], mr.ORDER0, 14),
              mr.w3_model(w3, L3, mr.ORDER0, 14, (A0, A1, A0)), w3.APM(w3.APM(w3.APM(o012, *A0), *A1), *A0)):   # three APM stages
        assert covers(m) is False
    lib = L.load()
    bad = L.ModelSpec()
    bad.n_nodes = 1
    bad.nodes[0].kind = L.W3_NODE_BEST_OF_TWO   # nothing to pop
    assert lib.w3_decode_spec_covers(C.byref(bad)) == lib.w3_spec_validate(C.byref(bad)) == L.W3_E_INVALID
    frozen = L.ModelSpec()   # a valid shape that is not built: a frozen leaf under a mixer
    frozen.n_nodes = 3
    for i, (kind, bits, align, max_bits, fr) in enumerate(((L.W3_NODE_ORDERN, 11, 3, 0, 0), (L.W3_NODE_ORDERN, 19, 3, 0, 1), (L.W3_NODE_MIX, 2, L.W3_MIX_ORDER0, 14, 0))):
        nd = frozen.nodes[i]
        nd.kind, nd.bits, nd.align, nd.max_bits, nd.frozen = kind, bits, align, max_bits, fr
    assert lib.w3_decode_spec_covers(C.byref(frozen)) == lib.w3_spec_validate(C.byref(frozen)) == L.W3_E_UNSUPPORTED
    with pytest.raises(w3.W3Error) as e:
        covers(bad)
    assert e.value.code == L.W3_E_INVALID
