"""Directed tests of the lane-per-block kernels (csrc/w3_generic.h, csrc/w3_cm.h: eleven instantiations per direction), one
model per form of the launch rule (lane_launch, w3hip.hip), by the rule itself and not by a variant:

  Counter leaves x1..4                  the batch form, every leaf count                      k_generic_nl<NL>
  Counter leaves x5, 9, 16              the run-time leaf loop; from 9 leaves on the lane kernels are the default decoder too   k_generic
  Counter x1..4 + 1 and 4 APM stages    batch form + APM chain, both row kinds, mixed rates   k_cm_nl<NL>
  Counter x5 + 1 APM stage              the staged kernel without a slot leaf                 k_cm_staged
  slot leaves x1, x8                    cells staged in LDS                                   k_cm_staged
  slot leaves x9 + Order0 + 2 APM       cells in global memory                                k_cm

Each: encoded on the lane-per-block path, lengths and bytes equal to the CPU oracle's; decoded by the default rule and by the lane
kernels.  66 blocks of 512 bytes: two wavefronts, the second ragged, and a short last block.  The Counter leaves are distinct, so each
can win the BestOfTwo choice; OrderN(22, 2) is an exact map at this block size; the slot leaves' tables are small enough to evict
within a block.  One range decode per family (Counter batch, Counter loop, slot) runs under decode_lane."""
import pytest

import weath3rb0i_amd as w3
from tests.synth import markov_text, mixed_bytes
from tests.test_gpu_parity import huff_pair
from tests.test_gpu_ranges import check_both, some_ranges

pytestmark = pytest.mark.gpu

BS = 512
DATA = markov_text(40 * BS) + mixed_bytes(25 * BS + 17)


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def counters(m, huff, n):
    """the first n of sixteen distinct Counter leaves: an exact map, alignment 0, a HuffHistory leaf and a FrozenModel among the first four"""
    pool = [lambda: m.OrderN(22, 2), lambda: m.OrderN(12, 0), lambda: m.OrderNEntropy(11, 3, huff), lambda: m.FrozenModel(m.Order1()),
            lambda: m.Order0(), lambda: m.Order1(), lambda: m.OrderN(9, 1), lambda: m.OrderN(14, 4), lambda: m.OrderN(10, 0),
            lambda: m.OrderN(16, 3), lambda: m.OrderN(8, 3), lambda: m.OrderN(11, 2), lambda: m.OrderN(13, 1), lambda: m.OrderN(18, 2),
            lambda: m.OrderN(20, 3), lambda: m.OrderN(15, 0)]
    return [f() for f in pool[:n]]


def slots(m, n):
    """n distinct slot-state leaves with tables of 16 to 64 cells"""
    return [m.SlotModel(k % 8, 4 + (k + 2 * (k // 8)) % 3) for k in range(n)]


def tree(m, leaves):
    t = leaves[0]
    for leaf in leaves[1:]:
        t = m.BestOfTwoModel(t, leaf)
    return t


def apm(m, t, stages):
    for kind, rate in [(0, 7), (1, 6), (0, 5), (1, 4)][:stages]:
        t = m.APM(t, kind, rate)
    return t


CASES = {}
for _n in (1, 2, 3, 4, 5, 9, 16):
    CASES["counter%d" % _n] = lambda m, h, n=_n: tree(m, counters(m, h, n))
for _n in (1, 2, 3, 4):
    CASES["counter%d_apm1" % _n] = lambda m, h, n=_n: m.APM(tree(m, counters(m, h, n)), n & 1, 5 + n)   # (both row kinds over the four)
    CASES["counter%d_apm4" % _n] = lambda m, h, n=_n: apm(m, tree(m, counters(m, h, n)), 4)
CASES["counter5_apm1"] = lambda m, h: apm(m, tree(m, counters(m, h, 5)), 1)
CASES["slot1"] = lambda m, h: m.SlotModel(2, 5)
CASES["slot8"] = lambda m, h: tree(m, slots(m, 8))
CASES["slot9_order0_apm2"] = lambda m, h: apm(m, tree(m, slots(m, 5) + [m.Order0()] + slots(m, 9)[5:]), 2)


def models(oracle, name):
    dev_h, orc_t = huff_pair(oracle)
    return CASES[name](w3, dev_h), CASES[name](oracle, oracle.HuffHistory(tables=orc_t))


def encode_lane(ctx, model):
    ctx.set_path("generic")
    try:
        out, lens = ctx.encode_blocks(model, DATA, BS)
        assert ctx.timing()["path"] == 1
    finally:
        ctx.set_path("auto")
    return out, lens


@pytest.mark.parametrize("name", list(CASES))
def test_lane_kernel_forms(ctx, oracle, name):
    dev, orc = models(oracle, name)
    out, lens = encode_lane(ctx, dev)
    want, wlens = oracle.encode_blocks(orc, DATA, BS, nthreads=8)
    assert lens.tolist() == wlens.tolist(), name
    assert out.tobytes() == want.tobytes(), name
    assert ctx.decode_blocks(dev, out, lens, BS, len(DATA)).tobytes() == DATA, name + " (default decoder)"
    ctx.set_variant("decode_lane")
    try:
        assert ctx.decode_blocks(dev, out, lens, BS, len(DATA)).tobytes() == DATA, name + " (lane-per-block decoder)"
    finally:
        ctx.set_variant()


@pytest.mark.parametrize("name", ["counter3_apm4", "counter9", "slot9_order0_apm2"])
def test_lane_kernel_range_decode(ctx, oracle, name):
    """ranges that start and end inside blocks (the kernels' job prefix), against slices of the input"""
    dev, _ = models(oracle, name)
    out, lens = encode_lane(ctx, dev)
    ctx.set_variant("decode_lane")
    try:
        check_both(ctx, dev, DATA, out, lens, BS, some_ranges(len(DATA), BS, seed=7))
    finally:
        ctx.set_variant()
