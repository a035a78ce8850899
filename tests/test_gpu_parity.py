"""GPU parity: the HIP path (through the C ABI) against the CPU oracle, byte for byte."""
import hashlib

import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests.synth import lcg_text, markov_text, mixed_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


_HUFF = {}


def huff_pair(oracle, key="text"):
    """One HuffHistory table set on both sides, from the oracle's package-merge (the device gets the tables across the ABI):
    trained on text (typical code lengths) or on a skewed buffer (1-bit codes, zero-count symbols: len 0)."""
    if key not in _HUFF:
        train = markov_text(40000, seed=61) if key == "text" else (b"e" * 30000 + b" " * 9000 + b"tao" * 700)
        t = oracle.huff_tables(train, 12, 12)
        dev = w3.HuffHistory.from_tables(list(t.code), list(t.len), list(t.rem_code), list(t.rem_len))
        _HUFF[key] = (dev, t)
    return _HUFF[key]


def pair(oracle, name):
    """(device model, oracle model factory) for a named configuration."""
    if name.startswith("huff"):
        _, bits, key = name.split("_")
        dev_h, orc_t = huff_pair(oracle, key)
        if bits == "mix":
            return (lambda: w3.BestOfTwoModel(w3.Order0(), w3.BestOfTwoModel(w3.OrderNEntropy(11, 3, dev_h), w3.OrderNEntropy(10, 3, huff_pair(oracle, "skew")[0]))),
                    lambda: oracle.BestOfTwoModel(oracle.Order0(), oracle.BestOfTwoModel(oracle.OrderNEntropy(11, 3, oracle.HuffHistory(tables=orc_t)),
                                                                                         oracle.OrderNEntropy(10, 3, oracle.HuffHistory(tables=huff_pair(oracle, "skew")[1])))))
        return (lambda: w3.OrderNEntropy(int(bits), 3, dev_h), lambda: oracle.OrderNEntropy(int(bits), 3, oracle.HuffHistory(tables=orc_t)))
    book1 = [1, 50188, 62497, 15819, 22545, 31499, 22988, 29616]
    enwik7 = [752, 50314, 58928, 21421, 24680, 30788, 24297, 32530]
    edge = [0, 65535, 1, 32768, 0, 65535, 12345, 1]
    table = {
        "order0": (lambda: w3.Order0(), lambda: oracle.Order0()),
        "order1": (lambda: w3.Order1(), lambda: oracle.Order1()),
        "order2": (lambda: w3.OrderN(27, 3), lambda: oracle.OrderN(27, 3)),
        "ordern_12_0": (lambda: w3.OrderN(12, 0), lambda: oracle.OrderN(12, 0)),
        "ordern_14_4": (lambda: w3.OrderN(14, 4), lambda: oracle.OrderN(14, 4)),
        "ordern_9_1": (lambda: w3.OrderN(9, 1), lambda: oracle.OrderN(9, 1)),
        "ordern_8_3": (lambda: w3.OrderN(8, 3), lambda: oracle.OrderN(8, 3)),
        "ordern_22_2": (lambda: w3.OrderN(22, 2), lambda: oracle.OrderN(22, 2)),
        "ordern_30_3": (lambda: w3.OrderN(30, 3), lambda: oracle.OrderN(30, 3)),
        "raw_16_3": (lambda: w3.OrderNEntropy(16, 3, w3.RawHistory()), lambda: oracle.OrderNEntropy(16, 3, oracle.RawHistory())),
        "raw_29_3": (lambda: w3.OrderNEntropy(29, 3, w3.RawHistory()), lambda: oracle.OrderNEntropy(29, 3, oracle.RawHistory())),
        "ordern_30_1": (lambda: w3.OrderN(30, 1), lambda: oracle.OrderN(30, 1)),
        "ordern_32_1": (lambda: w3.OrderN(32, 1), lambda: oracle.OrderN(32, 1)),   # the reference's best plain configuration (bin/ordern/enwik7.log:163)
        # the reference's best ratios: bin/entropy-hashing-ac/main.rs:21-25 (26,3)+ACHistory(23, enwik7) / (20,3)+ACHistory(17, book1)
        "ac_26_3_mb23_enwik7": (lambda: w3.OrderNEntropy(26, 3, w3.ACHistory(23, w3.StationaryModel.for_enwik7())),
                                lambda: oracle.OrderNEntropy(26, 3, oracle.ACHistory(23, oracle.StationaryModel.from_table(enwik7)))),
        "ac_20_3_mb17_book1": (lambda: w3.OrderNEntropy(20, 3, w3.ACHistory(17, w3.StationaryModel.for_book1())),
                               lambda: oracle.OrderNEntropy(20, 3, oracle.ACHistory(17, oracle.StationaryModel.from_table(book1)))),
        "best_wave_mix": (lambda: w3.BestOfTwoModel(w3.Order0(), w3.BestOfTwoModel(w3.OrderN(22, 2), w3.BestOfTwoModel(w3.Order1(), w3.OrderNEntropy(20, 3, w3.ACHistory(17, w3.StationaryModel.for_book1()))))),
                          lambda: oracle.BestOfTwoModel(oracle.Order0(), oracle.BestOfTwoModel(oracle.OrderN(22, 2), oracle.BestOfTwoModel(oracle.Order1(), oracle.OrderNEntropy(20, 3, oracle.ACHistory(17, oracle.StationaryModel.from_table(book1))))))),
        "main_default": (lambda: w3.init_model(),
                         lambda: oracle.OrderNEntropy(11, 3, oracle.ACHistory(8, oracle.StationaryModel.from_table(book1)))),
        "ac_19_3_enwik7": (lambda: w3.OrderNEntropy(19, 3, w3.ACHistory(16, w3.StationaryModel.for_enwik7())),
                           lambda: oracle.OrderNEntropy(19, 3, oracle.ACHistory(16, oracle.StationaryModel.from_table(enwik7)))),
        "ac_10_2_mb0": (lambda: w3.OrderNEntropy(10, 2, w3.ACHistory(0, w3.StationaryModel.for_book1())),
                        lambda: oracle.OrderNEntropy(10, 2, oracle.ACHistory(0, oracle.StationaryModel.from_table(book1)))),
        "ordern_5_3": (lambda: w3.OrderN(5, 3), lambda: oracle.OrderN(5, 3)),
        "ordern_3_3": (lambda: w3.OrderN(3, 3), lambda: oracle.OrderN(3, 3)),
        "ordern_10_3": (lambda: w3.OrderN(10, 3), lambda: oracle.OrderN(10, 3)),
        "ac_7_3_mb4": (lambda: w3.OrderNEntropy(7, 3, w3.ACHistory(4, w3.StationaryModel.for_enwik7())),
                       lambda: oracle.OrderNEntropy(7, 3, oracle.ACHistory(4, oracle.StationaryModel.from_table(enwik7)))),
        "ac_11_3_mb16": (lambda: w3.OrderNEntropy(11, 3, w3.ACHistory(16, w3.StationaryModel.for_book1())),
                         lambda: oracle.OrderNEntropy(11, 3, oracle.ACHistory(16, oracle.StationaryModel.from_table(book1)))),
        # extreme StationaryModel tables: prob 0 (lerp operand 1: up to 32 bits per coded history bit), 65535, 1, one half
        "ac_edge_table_mb8": (lambda: w3.OrderNEntropy(11, 3, w3.ACHistory(8, w3.StationaryModel.from_table(edge))),
                              lambda: oracle.OrderNEntropy(11, 3, oracle.ACHistory(8, oracle.StationaryModel.from_table(edge)))),
        "ac_edge_table_mb32": (lambda: w3.OrderNEntropy(11, 3, w3.ACHistory(32, w3.StationaryModel.from_table(edge))),
                               lambda: oracle.OrderNEntropy(11, 3, oracle.ACHistory(32, oracle.StationaryModel.from_table(edge)))),
        "best_frozen_first": (lambda: w3.BestOfTwoModel(w3.FrozenModel(w3.Order1()), w3.Order0()),
                              lambda: oracle.BestOfTwoModel(oracle.FrozenModel(oracle.Order1()), oracle.Order0())),
        "best_ac_wide": (lambda: w3.BestOfTwoModel(w3.init_model(), w3.BestOfTwoModel(w3.OrderN(27, 3), w3.Order1())),
                         lambda: oracle.BestOfTwoModel(oracle.OrderNEntropy(11, 3, oracle.ACHistory(8, oracle.StationaryModel.from_table(book1))),
                                                       oracle.BestOfTwoModel(oracle.OrderN(27, 3), oracle.Order1()))),
        "frozen0": (lambda: w3.FrozenModel(w3.Order0()), lambda: oracle.FrozenModel(oracle.Order0())),
        "best01": (lambda: w3.BestOfTwoModel(w3.Order0(), w3.Order1()), lambda: oracle.BestOfTwoModel(oracle.Order0(), oracle.Order1())),
        "best012": (lambda: w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3)),
                    lambda: oracle.BestOfTwoModel(oracle.BestOfTwoModel(oracle.Order0(), oracle.Order1()), oracle.OrderN(27, 3))),
        "best_right": (lambda: w3.BestOfTwoModel(w3.Order1(), w3.BestOfTwoModel(w3.FrozenModel(w3.Order0()), w3.Order0())),
                       lambda: oracle.BestOfTwoModel(oracle.Order1(), oracle.BestOfTwoModel(oracle.FrozenModel(oracle.Order0()), oracle.Order0()))),
    }
    return table[name]


def check_blocks(ctx, oracle, name, data, bs, path):
    dev, orc = pair(oracle, name)
    ctx.set_path(path)
    try:
        out, lens = ctx.encode_blocks(dev(), data, bs)
    finally:
        ctx.set_path("auto")
    want, wlens = oracle.encode_blocks(orc(), data, bs, nthreads=8)
    assert lens.tolist() == wlens.tolist(), (name, path)
    assert out.tobytes() == want.tobytes(), (name, path)
    return out, lens


def decode_both(ctx, model, out, lens, bs, n, forms=4):
    """Decode with the default kernels (k_decode_spec: sixteen lanes per block, where it applies) and with the lane-per-block kernels
    (W3_OPT_VARIANT decode_lane); both must agree — and so must k_decode_spec's other forms (two-bit groups, the nibble-major table
    formats of large batches with the all-raw-history instance and with the general kernel)."""
    a = ctx.decode_blocks(model, out, lens, bs, n).tobytes()
    if forms <= 1:   # (blocks of several MiB: the lane-per-block decoder alone takes half a minute per block)
        return np.frombuffer(a, dtype=np.uint8)
    ctx.set_variant("decode_lane")
    try:
        b = ctx.decode_blocks(model, out, lens, bs, n).tobytes()
    finally:
        ctx.set_variant()
    assert a == b, "k_decode_spec and the lane-per-block decoder disagree"
    if forms <= 2:   # (blocks of several MiB: a decode is one latency chain per block, tens of seconds each)
        return np.frombuffer(a, dtype=np.uint8)
    ctx.set_tune(16384)   # k_decode_spec with two bits per speculated group (four lanes per block: the form of large batches)
    try:
        c = ctx.decode_blocks(model, out, lens, bs, n).tobytes()
    finally:
        ctx.set_tune(0)
    assert a == c, "k_decode_spec: the two-bit groups and the nibble groups disagree"
    ctx.set_tune(262144)   # k_decode_spec with the nibble-major table formats of large batches (bucketed exact maps, APM tables by nibble group)
    try:
        d = ctx.decode_blocks(model, out, lens, bs, n).tobytes()
    finally:
        ctx.set_tune(0)
    assert a == d, "k_decode_spec: the nibble-major table formats and the round-3 formats disagree"
    ctx.set_tune(262144 | 524288)   # the same with the general kernel where the all-raw-history instance would run (bit 19)
    try:
        e = ctx.decode_blocks(model, out, lens, bs, n).tobytes()
    finally:
        ctx.set_tune(0)
    assert a == e, "k_decode_spec: the all-raw instance and the general kernel disagree"
    return np.frombuffer(a, dtype=np.uint8)


ALL = ["order0", "order1", "order2", "ordern_12_0", "ordern_14_4", "ordern_9_1", "ordern_8_3", "ordern_22_2", "ordern_30_3",
       "raw_16_3", "main_default", "ac_19_3_enwik7", "ac_10_2_mb0", "frozen0", "best01", "best012", "best_right",
       "huff_11_text", "huff_19_text", "huff_24_text", "huff_11_skew", "huff_mix_text"]


TWOPHASE = ["order0", "order1", "order2", "ordern_8_3", "ordern_5_3", "ordern_3_3", "ordern_10_3", "main_default", "ac_7_3_mb4",
            "ac_11_3_mb16", "ac_edge_table_mb8", "ac_edge_table_mb32", "frozen0", "best01", "best012", "best_right", "best_frozen_first",
            "best_ac_wide", "huff_11_text", "huff_7_text", "huff_11_skew", "huff_mix_text"]
# any other Counter-table leaf: wave per block, table in HBM (k_predict_wave) — lane-per-block kernel before round 3
WAVE = ["ordern_12_0", "ordern_14_4", "ordern_9_1", "ordern_22_2", "ordern_30_3", "ordern_30_1", "ordern_32_1", "raw_16_3", "raw_29_3", "ac_19_3_enwik7",
        "ac_26_3_mb23_enwik7", "ac_20_3_mb17_book1", "ac_10_2_mb0", "huff_19_text", "huff_24_text", "huff_19_skew", "best_wave_mix"]


def test_counter_p_exhaustive(ctx):
    import ctypes as C
    bad = C.c_uint64(123)
    assert ctx.lib.w3_selftest_counter_p(ctx.h, C.byref(bad)) == 0
    assert bad.value == 0


@pytest.mark.parametrize("name", ALL)
def test_generic_path_all_models(ctx, oracle, name):
    data = markov_text(40000, seed=11) + lcg_text(9000, seed=2)
    out, lens = check_blocks(ctx, oracle, name, data, 4096, "generic")
    dev, orc = pair(oracle, name)
    back = decode_both(ctx, dev(), out, lens, 4096, len(data))
    assert back.tobytes() == data


@pytest.mark.parametrize("name", TWOPHASE)
def test_twophase_path_models(ctx, oracle, name):
    data = markov_text(70000, seed=12) + lcg_text(9000, seed=3) + bytes(3000) + markov_text(5000, seed=13)
    out, lens = check_blocks(ctx, oracle, name, data, 16384, "twophase")
    assert ctx.timing()["path"] == 2
    # Model::predict for every step, straight from the predict kernels
    dev, orc = pair(oracle, name)
    p = ctx.predict_blocks(dev(), data[:40000], 16384)
    want = np.concatenate([oracle.predict_all(orc(), data[o:min(o + 16384, 40000)]) for o in range(0, 40000, 16384)])
    assert np.array_equal(p, want)


def test_huff_keys_long_run_of_untrained_byte(ctx, oracle):
    """A byte absent from HuffHistory's training buffer has code length 0 (legal through from_tables): it adds nothing to
    compressed_bits, so k_huffkeys' walk-back over a long run of it never covers 32 bits.  The walk is bounded and such blocks
    are redone with the forward recurrence (k_huffkeys_fix): a 64 KiB block that is ONE run of an untrained byte must come out
    exact, in well under a second (the unbounded walk was ~2^31 loads for it), and so must runs that start mid-block."""
    import time
    data = b"x" * 65536 + markov_text(3000, seed=5) + b"\x00" * 40000 + b"e tao" * 2000 + b"x" * 30000 + markov_text(2000, seed=6)
    t0 = time.time()
    check_blocks(ctx, oracle, "huff_11_skew", data, 65536, "twophase")
    check_blocks(ctx, oracle, "huff_mix_text", data, 16384, "twophase")
    assert time.time() - t0 < 60
    dev, orc = pair(oracle, "huff_11_skew")
    p = ctx.predict_blocks(dev(), data[:70000], 65536)
    want = np.concatenate([oracle.predict_all(orc(), data[o:min(o + 65536, 70000)]) for o in range(0, 70000, 65536)])
    assert np.array_equal(p, want)


def test_order2_partition_chained_and_from_scratch(ctx, oracle):
    """An order-2 leaf behind an Order1 leaf refines that leaf's c1-sorted records (k_partition<3>, two passes); alone,
    ahead of the Order1 leaf, or with the hook set it sorts from scratch (k_partition<2>, four passes).  Same streams."""
    data = markov_text(150000, seed=21) + bytes(70000) + lcg_text(30001, seed=4)
    for name in ("best012", "best_ac_wide", "order2"):
        check_blocks(ctx, oracle, name, data, 65536, "twophase")
    try:
        ctx.set_variant("no_chained_partition")
        check_blocks(ctx, oracle, "best012", data, 65536, "twophase")
        ctx.set_variant("partition4")                            # 4-bit LSD passes (k_partition<1>, <3>) instead of k_partition8
        check_blocks(ctx, oracle, "best012", data, 65536, "twophase")
        ctx.set_variant("no_side_stream")
        check_blocks(ctx, oracle, "best012", data, 65536, "twophase")
    finally:
        ctx.set_variant()


def test_ballot_rounds_without_lds_atomics(oracle):
    """A device that fails the lane-order self-test of returning LDS adds (forced with W3_OPT_VARIANT) runs the ballot
    rounds and the 4-bit partition passes everywhere: same streams."""
    c = w3.Context(0)
    c.set_variant("no_lds_atomics")
    try:
        data = markov_text(150000, seed=22) + bytes(66000) + lcg_text(9000, seed=5)
        for name in ("order0", "best012", "main_default", "best_ac_wide"):
            check_blocks(c, oracle, name, data, 65536, "twophase")
    finally:
        c.close()


def test_sharded_encode_from_one_process(oracle):
    """w3_encode_blocks_sharded: contiguous block ranges on several contexts (here three on the one GPU of the box), one host
    thread each; streams and length table identical to the single-context call, also when ranges are empty."""
    import ctypes as C
    from weath3rb0i_amd import _lib as L
    cs = [w3.Context(0) for _ in range(3)]
    try:
        for n in (150000, 4096 * 2 + 5, 100):
            data = np.frombuffer(markov_text(n, seed=27), dtype=np.uint8)
            bs = 4096
            nb = (n + bs - 1) // bs
            model = w3.BestOfTwoModel(w3.Order0(), w3.Order1())
            want, wlens = cs[0].encode_blocks(model, data, bs)
            spec = model.spec()
            hs = (C.c_void_p * 3)(*[c.h for c in cs])
            out = np.zeros(2 * n + 64 * nb + 64, dtype=np.uint8)
            lens = np.zeros(nb, dtype=np.uint32)
            olen = C.c_size_t()
            rc = cs[0].lib.w3_encode_blocks_sharded(hs, 3, C.byref(spec), data.ctypes.data_as(C.c_void_p), n, bs, out.ctypes.data_as(C.c_void_p),
                                                    len(out), C.byref(olen), lens.ctypes.data_as(C.c_void_p))
            assert rc == 0, cs[0].lib.w3_last_error(cs[0].h)
            assert lens.tolist() == wlens.tolist() and out[:olen.value].tobytes() == want.tobytes()
    finally:
        for c in cs:
            c.close()


def test_sharded_encode_device_resident_gather(oracle):
    """w3_encode_blocks_sharded_device: shards resident on the devices, streams and length table gathered on the root's device.
    On the 1-GPU box: three contexts on the one device (device-copy transport; ranges may be empty), and ONE context through the
    RCCL transport (ncclCommInitAll with one rank + the sizes all-gather: the lazily resolved librccl really loads and runs).
    Output identical to the single-context call over the concatenated shards."""
    import ctypes as C
    import torch
    from weath3rb0i_amd import _lib as L
    cs = [w3.Context(0) for _ in range(3)]
    try:
        bs = 4096
        model = w3.BestOfTwoModel(w3.Order0(), w3.Order1())
        for n in (150000, 4096 * 2 + 5, 100):
            data = np.frombuffer(markov_text(n, seed=28), dtype=np.uint8).copy()
            nb = (n + bs - 1) // bs
            want, wlens = cs[0].encode_blocks(model, data, bs)
            d_out = torch.empty(2 * n + 64 * nb + 64, dtype=torch.uint8, device="cuda")
            d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
            for k, transport, root in ((3, "auto", 0), (3, "peer_copy", 2), (1, "rccl", 0)):
                d_out.zero_(); d_lens.zero_()
                shards = []
                for r in range(k):
                    b0, b1 = C.c_size_t(), C.c_size_t()
                    assert cs[0].lib.w3_shard_range(nb, k, r, C.byref(b0), C.byref(b1)) == 0
                    shards.append(torch.from_numpy(data[min(b0.value * bs, n):min(b1.value * bs, n)].copy()).cuda())
                torch.cuda.synchronize()
                totals = w3.encode_blocks_sharded_device(cs[:k], model, shards, bs, d_out, d_lens, root=root, transport=transport)
                assert sum(totals) == len(want), (n, k, transport)
                assert d_lens.cpu().numpy().astype(np.uint32).tolist() == wlens.tolist(), (n, k, transport)
                assert d_out[: len(want)].cpu().numpy().tobytes() == want.tobytes(), (n, k, transport)
        # errors: RCCL transport with contexts that share a device; a middle shard that is not a whole number of blocks; out_cap
        shards = [torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(100, dtype=torch.uint8, device="cuda")]
        with pytest.raises(w3.W3Error) as e:
            w3.encode_blocks_sharded_device(cs[:2], model, shards, bs, d_out, d_lens, transport="rccl")
        assert e.value.code == L.W3_E_INVALID
        with pytest.raises(w3.W3Error) as e:
            w3.encode_blocks_sharded_device(cs[:2], model, shards[::-1], bs, d_out, d_lens)
        assert e.value.code == L.W3_E_INVALID
        with pytest.raises(w3.W3Error) as e:
            w3.encode_blocks_sharded_device(cs[:2], model, shards, bs, d_out[:3], d_lens)
        assert e.value.code == L.W3_E_NOSPACE
    finally:
        for c in cs:
            c.close()


def test_sampled_verification_catches_misordered_lds_adds(oracle):
    """VERDICT r1 #5 / ADVICE: the default predict kernels rely on returning LDS adds resolving in lane order (measured, not in
    the ISA manual).  Every call re-predicts sampled blocks with ballot rounds and compares (W3_OPT_VERIFY).  With the fault
    hook one LDS-add round of every block is corrupted: the verification must notice, the call must still return the
    oracle's streams (re-encoded on the ballot path) and the context must stay on that path."""
    data = markov_text(300000, seed=23) + lcg_text(30000, seed=6)
    for name in ("order0", "best012", "main_default"):
        c = w3.Context(0)
        try:
            c.set_path("twophase")
            dev, orc = pair(oracle, name)
            want, wlens = oracle.encode_blocks(orc(), data, 16384, nthreads=8)
            out, lens = c.encode_blocks(dev(), data, 16384)                    # clean run: verification on, nothing found
            assert c.timing()["n_lds_faults"] == 0 and out.tobytes() == want.tobytes()
            c.set_variant("inject_lds_fault")
            out, lens = c.encode_blocks(dev(), data, 16384)
            assert c.timing()["n_lds_faults"] > 0, name
            assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes(), name
            out, lens = c.encode_blocks(dev(), data, 16384)                    # the context now runs ballot rounds: no fault to find
            assert c.timing()["n_lds_faults"] == 0 and out.tobytes() == want.tobytes()
            c.set_variant("inject_lds_fault")                                  # (set_variant re-arms the LDS-add path)
            p = c.predict_blocks(dev(), data[:65536], 16384)                   # Model::predict straight from the kernels (no verification
            ref = np.concatenate([oracle.predict_all(orc(), data[o:o + 16384]) for o in range(0, 65536, 16384)])   # there): the corruption shows
            assert not np.array_equal(p, ref), name
            with pytest.raises(w3.W3Error):                                    # the hook cannot be used to corrupt OUTPUT: it needs the verification
                c.set_verify(False)
        finally:
            c.close()


def test_sampled_verification_rotates_over_all_blocks(oracle):
    """The sample is max(16, nblocks / 256) blocks and ROTATES from call to call: a fault confined to ONE block that the first
    call's sample misses is met after a bounded number of calls (ceil(nblocks / sample): w3_verify.h; every block, whatever the block
    count, tests/test_gpu_lds_fault.py).  Until then the corrupted stream goes out —
    the coverage limit of a sampled check, stated in w3hip.h; the full check is a decode of the output (bench.py --full, test_gpu_fullsize)."""
    bs, nb = 1024, 400
    data = markov_text(bs * nb, seed=29)
    c = w3.Context(0)
    try:
        c.set_path("twophase")
        dev, orc = pair(oracle, "order0")
        want, wlens = oracle.encode_blocks(orc(), data, bs, nthreads=8)
        gap = nb // 16                      # 16 sampled blocks; slot s covers blocks [25 s, 25 s + 25) and call k takes 25 s + (k mod 25)
        victim = 25 * 3 + 7                 # first in the sample at call 7
        c.set_variant("inject_lds_fault")
        c.set_fault_block(victim)
        caught_at = None
        for call in range(gap + 1):
            out, lens = c.encode_blocks(dev(), data, bs)
            if c.timing()["n_lds_faults"] > 0:
                caught_at = call
                assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes()   # re-encoded on the ballot path
                break
            assert out.tobytes() != want.tobytes()   # not sampled yet: the one corrupted block goes out
        assert caught_at == 7, caught_at
        out, lens = c.encode_blocks(dev(), data, bs)   # the context stays on the ballot path
        assert c.timing()["n_lds_faults"] == 0 and out.tobytes() == want.tobytes()
    finally:
        c.close()


def _device_bufs(n, bs, count):
    import torch
    nb = (n + bs - 1) // bs
    return [(torch.empty(2 * n + 64 * nb + 64, dtype=torch.uint8, device="cuda"), torch.zeros(max(nb, 1), dtype=torch.int32, device="cuda"),
             torch.zeros(1, dtype=torch.int64, device="cuda")) for _ in range(count)]


def test_submit_wait_pipeline(ctx, oracle):
    """w3_encode_submit / w3_encode_wait: two calls in flight on one context (call k+1's predict phase beside call k's APM and
    coder kernels, each job in its own workspace, half-CU kernel shapes and k_coder_x5).  Every output equals the oracle's and the
    synchronous call's; jobs alternate over many submissions, with different inputs and specs in flight together; a third
    submission is refused until a job has been waited for; synchronous entry points are refused while jobs are in flight;
    specs outside the predict kernels run synchronously inside submit."""
    import torch
    from weath3rb0i_amd import _lib as L
    bs = 4096
    datas = [markov_text(300 * 1024 + 333, seed=31) + bytes(40 * 1024) + lcg_text(100 * 1024, seed=6), lcg_text(200 * 1024 + 7, seed=9) + markov_text(150 * 1024, seed=32)]
    names = ["best012", "order0", "main_default", "ordern_12_0"]   # the last one: lane-per-block kernel, synchronous inside submit
    d_ins = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in datas]
    bufs = _device_bufs(max(len(d) for d in datas), bs, 2)
    torch.cuda.synchronize()
    want = {(k, nm): oracle.encode_blocks(pair(oracle, nm)[1](), datas[k], bs, nthreads=8) for k in range(2) for nm in names}
    ctx.set_timing(True)
    ctx.set_tune(4096)   # the ordered pair of large inputs (inputs of this size would run as four free-running jobs: next test)
    try:
        pending = []   # (job, buffer index, data index, name)
        seq = [(i % 2, names[i % len(names)]) for i in range(10)]
        for i, (k, nm) in enumerate(seq):
            if len(pending) == 2:
                job, bi, kk, nn = pending.pop(0)
                ctx.encode_wait(job)
                d_out, d_lens, d_total = bufs[bi]
                w_out, w_lens = want[(kk, nn)]
                nbk = len(w_lens)
                assert d_lens[:nbk].cpu().numpy().astype(np.uint32).tolist() == w_lens.tolist(), (i, nn)
                assert d_out[: int(d_total.item())].cpu().numpy().tobytes() == w_out.tobytes(), (i, nn)
                assert ctx.timing()["total_ms"] > 0
            bi = i % 2
            job = ctx.encode_submit(pair(oracle, nm)[0](), d_ins[k], bs, *bufs[bi])
            pending.append((job, bi, k, nm))
            if len(pending) == 2 and i == 1:
                with pytest.raises(w3.W3Error) as e:   # both jobs busy
                    ctx.encode_submit(pair(oracle, nm)[0](), d_ins[k], bs, *bufs[bi])
                assert e.value.code == L.W3_E_INVALID
                with pytest.raises(w3.W3Error) as e:   # no synchronous call while jobs are in flight
                    ctx.encode_blocks(pair(oracle, "order0")[0](), datas[0][:9000], bs)
                assert e.value.code == L.W3_E_INVALID
        for job, bi, kk, nn in pending:
            ctx.encode_wait(job)
            d_out, d_lens, d_total = bufs[bi]
            w_out, w_lens = want[(kk, nn)]
            assert d_out[: int(d_total.item())].cpu().numpy().tobytes() == w_out.tobytes(), nn
        with pytest.raises(w3.W3Error):
            ctx.encode_wait(0)   # nothing in flight
    finally:
        ctx.set_timing(False)
        ctx.set_tune(0)
    # the rank kernels with eight wavefronts per half CU (4-round operand batches; W3_OPT_TUNE bit 15: measured slower, kept as a variant)
    ctx.set_tune(4096 | 32768)
    try:
        jobs = [ctx.encode_submit(pair(oracle, "best012")[0](), d_ins[k], bs, *bufs[k]) for k in range(2)]
        for k in range(2):
            ctx.encode_wait(jobs[k])
            assert bufs[k][0][: int(bufs[k][2].item())].cpu().numpy().tobytes() == want[(k, "best012")][0].tobytes(), k
    finally:
        ctx.set_tune(0)
    # the synchronous call in the pipeline's kernel shapes, and the submitted call in the plain shapes: same streams
    for variant in ("half_cu", "full_cu"):
        ctx.set_variant(variant)
        try:
            check_blocks(ctx, oracle, "best012", datas[0], bs, "twophase")
            job = ctx.encode_submit(pair(oracle, "best012")[0](), d_ins[0], bs, *bufs[0])
            ctx.encode_wait(job)
            assert bufs[0][0][: int(bufs[0][2].item())].cpu().numpy().tobytes() == want[(0, "best012")][0].tobytes(), variant
        finally:
            ctx.set_variant()


def test_submit_wait_four_free_running_jobs(ctx, oracle):
    """Inputs of at most 4,096 blocks (w3_encode_max_in_flight == 4): four submitted calls in flight, every code stage on its own
    stream so that the calls' coders overlap.  Different inputs and specs in flight together, waited for out of order, slots
    reused over many submissions; a fifth submission is refused; an ordered job (W3_OPT_TUNE bit 12) followed by free-running
    ones; every output equals the oracle's."""
    import torch
    from weath3rb0i_amd import _lib as L
    bs = 2048
    datas = [markov_text(200 * 1024 + 333, seed=41) + bytes(30 * 1024), lcg_text(150 * 1024 + 7, seed=19) + markov_text(90 * 1024, seed=42),
             markov_text(64 * 1024 + 1, seed=43)]
    names = ["best012", "o012_apm", "order0", "main_default", "apm_chain"]
    models = {"o012_apm": (lambda: w3.APM(w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3))),
                           lambda: oracle.APM(oracle.BestOfTwoModel(oracle.BestOfTwoModel(oracle.Order0(), oracle.Order1()), oracle.OrderN(27, 3)))),
              "apm_chain": (lambda: w3.APM(w3.APM(w3.Order1(), 0, 7), 1, 6), lambda: oracle.APM(oracle.APM(oracle.Order1(), 0, 7), oracle.APM_ORDER1, 6))}
    mk = lambda nm: models[nm] if nm in models else pair(oracle, nm)
    assert ctx.max_in_flight(len(datas[0]), bs) == 4 and ctx.max_in_flight(10**9, 65536) == 2 and ctx.max_in_flight(4096 * 65536, 65536) == 4 and ctx.max_in_flight(12288 * 65536, 65536) == 3 and ctx.max_in_flight(12289 * 65536, 65536) == 2
    d_ins = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in datas]
    bufs = _device_bufs(max(len(d) for d in datas), bs, 4)
    torch.cuda.synchronize()
    want = {(k, nm): oracle.encode_blocks(mk(nm)[1](), datas[k], bs, nthreads=8) for k in range(3) for nm in names}

    def finish(entry):
        job, bi, kk, nn = entry
        ctx.encode_wait(job)
        d_out, d_lens, d_total = bufs[bi]
        w_out, w_lens = want[(kk, nn)]
        assert d_lens[:len(w_lens)].cpu().numpy().astype(np.uint32).tolist() == w_lens.tolist(), (kk, nn)
        assert d_out[: int(d_total.item())].cpu().numpy().tobytes() == w_out.tobytes(), (kk, nn)

    rng = np.random.default_rng(5)
    pending, free = [], [0, 1, 2, 3]
    refused = False
    for i in range(22):
        if len(pending) == 4:
            if not refused:
                with pytest.raises(w3.W3Error) as e:   # all four slots busy
                    ctx.encode_submit(mk("order0")[0](), d_ins[0], bs, *bufs[0])
                assert e.value.code == L.W3_E_INVALID
                refused = True
            entry = pending.pop(int(rng.integers(0, len(pending))))   # any order
            finish(entry)
            free.append(entry[1])
        k, nm = i % 3, names[i % len(names)]
        bi = free.pop(0)
        if i == 9:
            while len(pending) > 1:   # (an ordered job is one of at most two in flight)
                entry = pending.pop(0)
                finish(entry)
                free.append(entry[1])
            ctx.set_tune(4096)    # one ordered job among the free-running ones: its code stage is enqueued by the next submit (or its wait)
        job = ctx.encode_submit(mk(nm)[0](), d_ins[k], bs, *bufs[bi])
        if i == 9:
            ctx.set_tune(0)
        assert 0 <= job < 4 and job not in [p[0] for p in pending]
        pending.append((job, bi, k, nm))
    for entry in reversed(pending):
        finish(entry)


def test_submit_wait_redo_paths(ctx, oracle):
    """What w3_encode_wait redoes synchronously: blocks the fast coder hands back (W3_OPT_ACC_LIMIT hook); and W3_E_NOSPACE.
    (A stripe overflow past 2N+64 takes the same redo; no adaptive-Counter input reaches it: the estimator's regret is bounded.)"""
    import torch
    from weath3rb0i_amd import _lib as L
    bs = 512
    data = markov_text(300 * 1024 + 333, seed=31) + bytes(40 * 1024) + lcg_text(200 * 1024, seed=6)
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    bufs = _device_bufs(len(data), bs, 2)
    w_out, w_lens = oracle.encode_blocks(pair(oracle, "best012")[1](), data, bs, nthreads=8)
    ctx.set_acc_limit(19)   # hand-backs in many blocks
    try:
        jobs = [ctx.encode_submit(pair(oracle, "best012")[0](), d_in, bs, *bufs[k]) for k in range(2)]
        for k in range(2):
            ctx.encode_wait(jobs[k])
            assert bufs[k][0][: int(bufs[k][2].item())].cpu().numpy().tobytes() == w_out.tobytes()
        assert ctx.timing()["n_recoded_blocks"] > 0
    finally:
        ctx.set_acc_limit(46)
    # out_cap too small: W3_E_NOSPACE from the wait, the need in d_total
    small = torch.empty(1000, dtype=torch.uint8, device="cuda")
    job = ctx.encode_submit(pair(oracle, "best012")[0](), d_in, bs, small, bufs[0][1], bufs[0][2])
    with pytest.raises(w3.W3Error) as e:
        ctx.encode_wait(job)
    assert e.value.code == L.W3_E_NOSPACE and int(bufs[0][2].item()) == len(w_out)


@pytest.mark.parametrize("name", WAVE)
def test_wave_per_block_predict_kernel(ctx, oracle, name):
    """k_predict_wave (w3_predict_wave.h): every Counter-table leaf outside the sorted kernels — any alignment_bits, hashed
    histories wider than 8 bits, 32-bit contexts through the exact map — on the two-phase path, bit-exact, Model::predict included."""
    data = markov_text(70000, seed=12) + lcg_text(9000, seed=3) + bytes(3000) + b"\xff" * 700 + markov_text(5000, seed=13)
    out, lens = check_blocks(ctx, oracle, name, data, 16384, "twophase")
    assert ctx.timing()["path"] == 2
    dev, orc = pair(oracle, name)
    back = decode_both(ctx, dev(), out, lens, 16384, len(data))
    assert back.tobytes() == data
    p = ctx.predict_blocks(dev(), data[:40000], 16384)
    want = np.concatenate([oracle.predict_all(orc(), data[o:min(o + 16384, 40000)]) for o in range(0, 40000, 16384)])
    assert np.array_equal(p, want)
    # ragged and tiny blocks, a block of one byte value (every step of a bit position on ONE Counter: the halving replay)
    for d_, bs_ in ((data[:8195], 4099), (data[:700], 9), (bytes(70000) + b"\xff" * 70000, 65536)):
        check_blocks(ctx, oracle, name, d_, bs_, "twophase")


def test_twophase_rejects_what_it_does_not_cover(ctx, oracle):
    """Inputs under 8 bytes (the window loads read 8 bytes at once) stay on the lane-per-block kernel."""
    from weath3rb0i_amd import _lib as L
    dev, _ = pair(oracle, "ordern_22_2")
    ctx.set_path("twophase")
    try:
        with pytest.raises(w3.W3Error) as e:
            ctx.encode_blocks(dev(), b"abcdefg", 64)
        assert e.value.code == L.W3_E_UNSUPPORTED
    finally:
        ctx.set_path("auto")
    out, lens = ctx.encode_blocks(dev(), b"abcdefg", 64)  # auto falls to the generic kernel
    assert ctx.timing()["path"] == 1
    check_blocks(ctx, oracle, "ordern_22_2", b"abcdefgh", 3, "twophase")


def saturation_cases():
    """Inputs whose Counters reach 65535 and halve (counter.rs:22-25): long constant runs, incl. multiple halvings.  -> {name: (data, bs)}"""
    rng = np.random.default_rng(5)
    z = bytearray(300000)
    for k in (70000, 140000, 141000, 290000):
        z[k] = 0x41
    cases = {
        "zeros64k": (bytes(65536), 65536), "ones64k": (b"\xff" * 65536, 65536), "zeros256k": (bytes(262144), 262144),
        "ones256k_ragged": (b"\xff" * 300001, 262144), "sparse": (bytes(z), 262144),
        "aa": (b"\xaa" * 200000, 131072), "ab": (b"ab" * 150000, 262144),
        "noisy_zero": (bytes(np.where(rng.random(262144) < 0.0005, 1, 0).astype(np.uint8)), 262144),
    }
    return cases


def test_twophase_counter_saturation(ctx, oracle):
    """Counter::update halves both counts at 65535 (counter.rs:22-25): long constant runs, incl. multiple halvings."""
    for cname, (data, bs) in saturation_cases().items():
        for name in ("order0", "best012", "main_default"):
            check_blocks(ctx, oracle, name, data, bs, "twophase")


def test_coder_variants_and_fallback(ctx, oracle):
    """Every coder kernel (k_coder_x4 / x5 asm pipelines, x3, x2, k_coder_fast with its slot/carry accumulator, the robust k_coder) and
    the hand-back path; x5, x4 and x3 also with one, three and four streams mixed on the fly (the mix and lane setup they share, at
    every L) and ragged / tiny blocks (the C paths x4 and x5 share: blocks below one chunk, below one ring, no multiple of either)."""
    data = markov_text(60000, seed=31) + bytes(5000) + np.random.default_rng(2).integers(0, 256, 20000, dtype=np.uint8).tobytes()
    want, wlens = oracle.encode_blocks(oracle.BestOfTwoModel(oracle.Order0(), oracle.Order1()), data, 8192, nthreads=8)
    model = w3.BestOfTwoModel(w3.Order0(), w3.Order1())
    ctx.set_path("twophase")
    try:
        for mode in ("x4", "x5", "x3", "x2", "fast", "robust"):
            ctx.set_coder(mode)
            out, lens = ctx.encode_blocks(model, data, 8192)
            assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes(), mode
            assert ctx.timing()["n_recoded_blocks"] == 0
        for mode in ("x4", "x5", "x3", "x2", "fast"):
            ctx.set_coder(mode)
            for limit in (19, 24, 33):  # force the fast coders to give blocks back to k_coder
                ctx.set_acc_limit(limit)
                out, lens = ctx.encode_blocks(model, data, 8192)
                assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes(), (mode, limit)
                if limit == 19:
                    assert ctx.timing()["n_recoded_blocks"] > 0
            ctx.set_acc_limit(46)
        tail = markov_text(3 * 8192 + 5, seed=77) + b"ab"
        for name in ("order0", "best012", "best_ac_wide"):
            dev, orc = pair(oracle, name)
            for d_, bs_ in ((data, 8192), (tail, 8192), (tail[:8195], 4099), (tail[:700], 7), (tail[:64 * 13 + 3], 13)):
                want_, wlens_ = oracle.encode_blocks(orc(), d_, bs_, nthreads=8)   # one reference for the three coders
                for mode in ("x5", "x4", "x3"):
                    ctx.set_coder(mode)
                    out, lens = ctx.encode_blocks(dev(), d_, bs_)
                    assert lens.tolist() == wlens_.tolist(), (mode, name, len(d_), bs_)
                    assert out.tobytes() == want_.tobytes(), (mode, name, len(d_), bs_)
    finally:
        ctx.set_acc_limit(46)
        ctx.set_coder("x4")
        ctx.set_path("auto")


def test_survey_digests_on_device(ctx, oracle):
    d = lcg_text(65536)
    for m, n, sha in [(w3.Order0(), 43693, "37791f2604aaa6d6a81de79dbeb80ef09e25581d28c95f5cd5b411848aa7c64d"),
                      (w3.Order1(), 49588, "5bceb3081cb21048473d483534b6f1cc901e1ac04fb1858ea303c994cf1fb7dc"),
                      (w3.BestOfTwoModel(w3.Order0(), w3.Order1()), 45259, "19da6b5f594baf1395037f6ea2c497a8a0740806e3ceede028d20e7b6c09b518")]:
        out, lens = ctx.encode_blocks(m, d, 65536)
        assert lens.tolist() == [n] and hashlib.sha256(out.tobytes()).hexdigest() == sha


@pytest.mark.parametrize("path", ["generic", "twophase"])
def test_edge_blocks(ctx, oracle, path):
    bs = 65536
    cases = {
        "zeros": bytes(bs),                 # Counter halving at 65535
        "ones": b"\xff" * bs,
        "alt55": b"\x55" * 5000,
        "single": b"A",
        "bs_plus_1": lcg_text(4097, seed=5),
        "bs_minus_1": lcg_text(4095, seed=6),
        "ragged": lcg_text(3 * 4096 + 17, seed=7),
        "random": np.random.default_rng(1).integers(0, 256, 20000, dtype=np.uint8).tobytes(),
    }
    assert ctx.encode_blocks(w3.Order0(), bytes(bs), bs)[0].tobytes() == b"\xff" * 16
    assert ctx.encode_blocks(w3.Order0(), b"\xff" * bs, bs)[0].tobytes() == b"\x00" * 16 + b"\x01"
    for cname, data in cases.items():
        b = bs if cname in ("zeros", "ones") else 4096
        if path == "twophase" and len(data) < 4:
            # the predict kernels read 4-byte windows: inputs under 4 bytes always take the generic kernel
            with pytest.raises(w3.W3Error):
                check_blocks(ctx, oracle, "order0", data, b, path)
            check_blocks(ctx, oracle, "order0", data, b, "auto")
            continue
        for name in ("order0", "best012"):
            out, lens = check_blocks(ctx, oracle, name, data, b, path)
            dev, _ = pair(oracle, name)
            assert decode_both(ctx, dev(), out, lens, b, len(data)).tobytes() == data, (cname, name)
    out, lens = ctx.encode_blocks(w3.Order0(), b"", 4096)
    assert len(out) == 0 and len(lens) == 0
    assert len(ctx.decode_blocks(w3.Order0(), b"", [], 4096, 0)) == 0


def test_nospace_and_errors(ctx):
    import ctypes as C
    from weath3rb0i_amd import _lib as L
    data = np.frombuffer(lcg_text(8192, seed=9), dtype=np.uint8)
    spec = w3.Order0().spec()
    out = np.zeros(100, dtype=np.uint8)
    lens = np.zeros(2, dtype=np.uint32)
    olen = C.c_size_t()
    rc = ctx.lib.w3_encode_blocks(ctx.h, C.byref(spec), data.ctypes.data_as(C.c_void_p), len(data), 4096,
                                  out.ctypes.data_as(C.c_void_p), 100, C.byref(olen), lens.ctypes.data_as(C.c_void_p))
    assert rc == L.W3_E_NOSPACE and olen.value > 100 and lens.sum() == olen.value
    with pytest.raises(w3.W3Error) as e:
        ctx.encode_blocks(w3.Order0(), data, 0)
    assert e.value.code == L.W3_E_INVALID
    # one call handles less than 4 GiB (a dispatch counts work-items in 32 bits): refused before any buffer is touched
    rc = ctx.lib.w3_encode_blocks_device(ctx.h, C.byref(spec), C.c_void_p(256), C.c_size_t(1 << 32), C.c_size_t(65536), C.c_void_p(256), C.c_size_t(100),
                                         C.c_void_p(256), C.c_void_p(256), None)
    assert rc == L.W3_E_UNSUPPORTED and b"4 GiB" in ctx.lib.w3_last_error(ctx.h)


def test_decode_rejects_inflated_length_table(ctx):
    """a length table that claims more compressed bytes than the buffer holds is refused (W3_E_FORMAT) before any
    read — host-buffer and device-resident entry points."""
    import torch
    from weath3rb0i_amd import _lib as L
    data = lcg_text(20000, seed=17)
    out, lens = ctx.encode_blocks(w3.Order0(), data, 4096)
    bad = lens.copy()
    bad[-1] += 100000
    with pytest.raises(w3.W3Error) as e:
        ctx.decode_blocks(w3.Order0(), out, bad, 4096, len(data))
    assert e.value.code == L.W3_E_FORMAT
    d_comp = torch.from_numpy(np.array(out)).cuda()
    d_back = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    with pytest.raises(w3.W3Error) as e:
        ctx.decode_blocks_device(w3.Order0(), d_comp, torch.from_numpy(bad.astype(np.int32)).cuda(), 4096, len(data), d_back)
    assert e.value.code == L.W3_E_FORMAT
    ctx.decode_blocks_device(w3.Order0(), d_comp, torch.from_numpy(lens.astype(np.int32)).cuda(), 4096, len(data), d_back)
    assert d_back.cpu().numpy().tobytes() == data


def test_encode_is_ordered_after_async_producer(ctx, oracle):
    """the input is produced by an asynchronous torch kernel on the default stream immediately before the call
    (stream handle 0 = the ctx's own blocking stream, ordered against the legacy default stream), and d_lens / d_total are
    zeroed the same way.  64 MB keeps the producer running while the encode kernels are enqueued."""
    import torch
    n, bs = 1 << 26, 65536
    nb = n // bs
    base = torch.from_numpy(np.frombuffer(markov_text(1 << 20, seed=41), dtype=np.uint8).copy()).cuda()
    d_in = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(n + n // 4 + 64 * nb + 1024, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for stream_arg in (None, 0):
        d_in.zero_()
        torch.cuda.synchronize()
        d_in.copy_(base.repeat(n >> 20) ^ 1)          # async: several kernels on the default stream
        d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.encode_blocks_device(w3.Order0(), d_in, bs, d_out, d_lens, d_total, stream=stream_arg)
        lens = d_lens.cpu().numpy().astype(np.uint32)
        host = d_in.cpu().numpy()
        for b in (0, nb // 2, nb - 1):
            want, wl = oracle.encode_blocks(oracle.Order0(), host[b * bs:(b + 1) * bs].tobytes(), bs)
            off = int(lens[:b].sum())
            assert wl.tolist() == [int(lens[b])] and d_out[off:off + int(lens[b])].cpu().numpy().tobytes() == want.tobytes(), (stream_arg, b)


def test_reference_container(ctx, oracle):
    d = markov_text(6000, seed=3)
    book1 = [1, 50188, 62497, 15819, 22545, 31499, 22988, 29616]
    want = oracle.compress(oracle.OrderNEntropy(11, 3, oracle.ACHistory(8, oracle.StationaryModel.from_table(book1))), d)
    got = ctx.compress(d)  # init_model() default, main.rs:151
    assert got == want and got[:4] == b"w30i"
    assert ctx.decompress(got) == d
    assert ctx.compress(b"") == oracle.compress(oracle.Order0(), b"")
    assert ctx.decompress(ctx.compress(b"")) == b""
    with pytest.raises(w3.W3Error) as e:
        ctx.decompress(b"w31i" + bytes(20))
    from weath3rb0i_amd import _lib as L
    assert e.value.code == L.W3_E_FORMAT


def test_mixed_bytes_256k_blocks(ctx, oracle):
    data = mixed_bytes(600000, seed=5)
    check_blocks(ctx, oracle, "best01", data, 262144, "generic")
    check_blocks(ctx, oracle, "best012", data, 262144, "twophase")


def test_device_resident_api(ctx, oracle):
    import torch
    data = markov_text(50000, seed=21)
    bs = 8192
    nb = (len(data) + bs - 1) // bs
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_out = torch.empty(2 * len(data) + 1024, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.encode_blocks_device(w3.Order0(), d_in, bs, d_out, d_lens, d_total, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want, wlens = oracle.encode_blocks(oracle.Order0(), data, bs)
    assert d_lens.cpu().numpy().astype(np.uint32).tolist() == wlens.tolist()
    tot = int(d_total.item())
    assert d_out[:tot].cpu().numpy().tobytes() == want.tobytes()
    d_back = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    ctx.decode_blocks_device(w3.Order0(), d_out, d_lens, bs, len(data), d_back)
    assert d_back.cpu().numpy().tobytes() == data


@pytest.mark.parametrize("bs", [1 << 20, (1 << 22) + 12345])
def test_large_blocks_twophase(ctx, oracle, bs):
    """Blocks far longer than the bench's 64 KiB (the two-phase path takes up to 16 MiB): positions beyond 16 bits in the records,
    Counter saturation inside long groups, slice boundaries from the bin table, APM batches — against the oracle, with a ragged
    last block; and the decoder's round trip."""
    from tests.synth import mixed_bytes
    data = markov_text(bs + bs // 3, seed=41) + mixed_bytes(bs // 2 + 777, seed=42)
    for name in ("best012", "order1"):
        out, lens = check_blocks(ctx, oracle, name, data, bs, "twophase")
        assert ctx.timing()["path"] == 2
    dev = lambda: w3.APM(w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3)))
    orc = lambda: oracle.APM(oracle.BestOfTwoModel(oracle.BestOfTwoModel(oracle.Order0(), oracle.Order1()), oracle.OrderN(27, 3)))
    out, lens = ctx.encode_blocks(dev(), data, bs)
    want, wlens = oracle.encode_blocks(orc(), data, bs, nthreads=8)
    assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes()
    # (the decoders' own cross-checks run at the smaller sizes; here the round trip of the encoder's long-block streams is the point)
    assert decode_both(ctx, dev(), out, lens, bs, len(data), forms=2 if bs <= (1 << 20) else 1).tobytes() == data
