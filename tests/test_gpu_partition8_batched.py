"""k_partition8's two tile paths — full tiles of 2048 records (one returning LDS add per record, every phase a batch of LDS operations)
and the ragged last tile of a block (the predicated rounds) — byte for byte against oracle.encode_blocks on the twophase path.
  Block sizes: a ragged-only block (1 .. 2047), exactly one full tile (2048), full tiles plus a 1-record ragged tile (2049, 4097),
several full tiles (4096, 65536), two full tiles and a ragged one short of full (6143), and the fault hook's threshold (127 / 128).
Every input spans at least three blocks and ends in a short one (block size 1 has no shorter block: nine blocks there, since the
twophase path takes no input under 8 bytes).
  Inputs: the extremes of what one round's 64 lanes can do to the bins (all on one address; two addresses; 64 different ones; runs
of eight), and random and text bytes.
  Each model's streams must also be those of the 4-bit passes (k_partition, set_variant("partition4")): an independent cross-check."""
import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests.synth import markov_text
from tests.test_gpu_parity import pair

pytestmark = pytest.mark.gpu

BLOCK_SIZES = [1, 63, 64, 65, 127, 128, 2047, 2048, 2049, 4096, 4097, 6143, 65536]
MODELS = ["order1", "order2", "best012"]


def _length(bs):
    """two full blocks and a short one"""
    return max(2 * bs + max(1, bs // 3), 9)


def _repeated(n):
    """one bin: every lane of every round on one address, ranks 0 .. 2047 in a single bin"""
    return b"e" * n


def _alternating(n):
    return (b"ab" * (n // 2 + 1))[:n]


def _cyclic(n):
    """every lane of a round in a different bin"""
    return (bytes(range(256)) * (n // 256 + 1))[:n]


def _runs_of_8(n):
    """8-lane runs per bin; the bin runs straddle tile edges"""
    return np.repeat(np.arange(256, dtype=np.uint8), 8).tobytes() * (n // 2048 + 1)


def _random(n):
    return np.random.default_rng(2048 + n).integers(0, 256, n, dtype=np.uint8).tobytes()


def _text(n):
    return markov_text(n, seed=17)


INPUTS = {"repeated": _repeated, "alternating": _alternating, "cyclic": _cyclic, "runs_of_8": _runs_of_8, "random": _random, "text": _text}

# the whole file's input stays small enough for the oracle side to take seconds
assert sum(_length(bs) for bs in BLOCK_SIZES) * len(INPUTS) < 4_000_000


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    c.set_path("twophase")
    yield c
    c.close()


def _same(got, want, what):
    assert got[1].tolist() == want[1].tolist(), what
    assert got[0].tobytes() == want[0].tobytes(), what


@pytest.mark.parametrize("kind", list(INPUTS))
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_streams_match_the_oracle(ctx, oracle, bs, kind):
    n = _length(bs)
    data = INPUTS[kind](n)[:n]
    assert len(data) == n and -(-n // bs) >= 3 and (bs == 1 or n % bs)
    try:
        for name in MODELS:
            dev, orc = pair(oracle, name)
            want = oracle.encode_blocks(orc(), data, bs, nthreads=8)
            ctx.set_variant()
            _same(ctx.encode_blocks(dev(), data, bs), want, (name, bs, kind))
            if name == "best012":
                ctx.set_variant("no_chained_partition")   # the order-2 leaf sorts from scratch
                _same(ctx.encode_blocks(dev(), data, bs), want, (name, bs, kind, "no_chained_partition"))
            ctx.set_variant("partition4")
            _same(ctx.encode_blocks(dev(), data, bs), want, (name, bs, kind, "partition4"))
    finally:
        ctx.set_variant()


@pytest.mark.parametrize("bs", [4096, 65536])
def test_half_cu_instances(oracle, bs):
    """The instances of four wavefronts per workgroup (the half-CU shapes of the pipeline, W3_OPT_TUNE bit 5): same streams."""
    n = _length(bs)
    data = _text(n)
    c = w3.Context(0)
    try:
        c.set_path("twophase")
        c.set_variant("half_cu")
        c.set_tune(32)
        for name in ("order1", "best012"):
            dev, orc = pair(oracle, name)
            _same(c.encode_blocks(dev(), data, bs), oracle.encode_blocks(orc(), data, bs, nthreads=8), (name, bs))
    finally:
        c.close()


@pytest.mark.parametrize("bs", [4096, 1000])
def test_injected_fault_is_caught_on_both_tile_paths(oracle, bs):
    """The hook (round 1 of a block's first tile: two lanes of one bin exchange their places) in a full tile (blocks of 4096 bytes:
    the ranks are exchanged) and in a ragged one (blocks of 1000 bytes: the slots): the sampled verification catches it and the call
    returns the oracle's streams.  A run of one byte over positions 56 .. 135 of every block makes the exchanged records share their
    Counter keys — records with different keys may be ranked in either order with the same predictions."""
    b = bytearray(markov_text(20 * bs + bs // 3, seed=23))
    for o in range(0, len(b), bs):
        k = len(b[o + 56:o + 136])
        b[o + 56:o + 56 + k] = b"e" * k
    data = bytes(b)
    for name in ("order1", "best012"):
        dev, orc = pair(oracle, name)
        want = oracle.encode_blocks(orc(), data, bs, nthreads=8)
        c = w3.Context(0)
        try:
            c.set_path("twophase")
            _same(c.encode_blocks(dev(), data, bs), want, (name, bs, "clean"))
            assert c.timing()["n_lds_faults"] == 0
            c.set_variant("inject_lds_fault")
            c.set_fault_kernels("partition8")
            got = c.encode_blocks(dev(), data, bs)
            assert c.timing()["n_lds_faults"] > 0, (name, bs)
            _same(got, want, (name, bs, "recovered"))   # re-encoded on the ballot path
            got = c.encode_blocks(dev(), data, bs)       # the context stays there: nothing to find
            assert c.timing()["n_lds_faults"] == 0
            _same(got, want, (name, bs, "after"))
        finally:
            c.close()
