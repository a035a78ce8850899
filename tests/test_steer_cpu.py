"""The steered inputs of tests/test_gpu_steer.py (tests/steer.py) checked against the CPU oracle alone: the conditions that keep the GPU
tests from passing vacuously.  Every input must reach what it is there for — the run lengths, the end-of-block pending counts, the
blocks that a 64-bit slot accumulator cannot hold — and is pinned by its sha256, so that these conditions and the GPU run speak of the
same bytes."""
import collections
import hashlib

import pytest

from oracle import pyoracle as orc
from tests import aoh_ref, steer
from tests.test_gpu_cm import pair as cm_pair
from tests.test_gpu_parity import pair as counter_pair

COUNTER_KINDS = ["coverage", "kept", "ends", "hold", "mixed", "anti"]
CM_KINDS = ["coverage", "kept", "ends"]
AOH_KINDS = ["runs", "hold"]

SHA256 = {
    ("order0", "coverage"): "cd9391e031a50e63bd05ddc40926cddd69a4a2443fe9adb7c94b8b7861f304a8",
    ("order0", "kept"): "bf2eaceb875a0d3b929ecd20ce17b9aa4d6d4b926b89bfee2fc6bcc3bd71badb",
    ("order0", "ends"): "9ea72dedb8502dc6807e6e3bc3da4fbba8894604e49b077919d494191a9c6f3d",
    ("order0", "hold"): "2e15df96ba509462d9e615ceb0a768e5e0efb69a7bb1d59f5b8a8cfacf09a54f",
    ("order0", "mixed"): "a2db1bc54ba4e977e871554b90fbc356aa4eccc58053ef46d1205e15fed383e1",
    ("order0", "anti"): "6d6d12515a10770198fa54fdb66b4e8973fbaa223614c0622c6dda39ebaa277b",
    ("best01", "coverage"): "287e39e37c2089e20e65a8b1102077cb7397a423b6d9eb6679c24bc87e27558b",
    ("best01", "kept"): "f497ee7817b720d0a6f622c580f1541140a6bab3d9bdedfd5c696f9277766491",
    ("best01", "ends"): "9a4212479cff4fdfb0c8c5e03183949550f39082627358eb186cdabaf891c29f",
    ("best01", "hold"): "44db4a82eeefbff4f5b85e445e91a97f308909d8ee0d8f1ae90923e53ed06d63",
    ("best01", "mixed"): "d0f5d4a6eca01718ed0c44f8657da5afcf9bacbc6aa5ae9ec565a42730987b11",
    ("best01", "anti"): "a3e36d775a65e9ab50427c950bba4ecb96675125f151603493cec1aa79a68114",
    ("best012", "coverage"): "05cb9b4a16605a5a0fbeba3327214ad0be6e8fb21712623d68f51775f60026fa",
    ("best012", "kept"): "f497ee7817b720d0a6f622c580f1541140a6bab3d9bdedfd5c696f9277766491",
    ("best012", "ends"): "9a4212479cff4fdfb0c8c5e03183949550f39082627358eb186cdabaf891c29f",
    ("best012", "hold"): "9f847c33e121ef085796c015f935a3ec326d17cb96469dc99e3be55bce6bbcbc",
    ("best012", "mixed"): "9f78b640bf1381f487a2d504cc122544b6e74d6a1a7b8b15ba96897a824adeb7",
    ("best012", "anti"): "a3e36d775a65e9ab50427c950bba4ecb96675125f151603493cec1aa79a68114",
    ("main_default", "coverage"): "2ce9b558db8e027ba0e07f6de1ceb2cc0fd3992c3c52c579c46c36724a14b67d",
    ("main_default", "kept"): "fb0c5b93d0c41b1130e62e1e02a13bafae8a83fcb01a096f23fc4f2295e43134",
    ("main_default", "ends"): "d2cc1b8d80f4fbe8ba2ab3e6d3cd7a804a622f8db5286fc8aae2a9dbcb73176b",
    ("main_default", "hold"): "c965222ba6f033c68b4e3fd06fa5141f24a97785d6f1e8d782a1932fab1cbc8f",
    ("main_default", "mixed"): "3136abbbfc224d105caaca78e98b714b6788d44cbcaee4ed35d005aee1c63655",
    ("main_default", "anti"): "7ef28e630d6e02f995fd75270629c2360733d15e9934dd30a7c920550152e2e1",
    ("best_ac_wide", "coverage"): "59ddca139fd0f8e5f796ed329bafe072382ec5ca1af8bb901431ec9dead537f9",
    ("best_ac_wide", "kept"): "f2842c266757ad1e8d4fee178c346d8418dab1cd0b313e764787765dda549702",
    ("best_ac_wide", "ends"): "8f0c10004ae4f41de5d946a01a49ca057340495ea17108e6f9d4340e8863db37",
    ("best_ac_wide", "hold"): "b909e902a2810208bb01ffe8d5394c0850876a57e340d49e8ed87e3db48d19f1",
    ("best_ac_wide", "mixed"): "c80fb6ea825ce7403dc81e97c10b2634f53c0d18f8d0073a45553e2fc52eca1c",
    ("best_ac_wide", "anti"): "64acaec8e927f4eb2f899e49b0605c6c4cb5777d3e6ba011060c0c46aacb49aa",
    ("o012_apm", "coverage"): "72ee9b76ba1c526435abade503165fe6d7251061fb12a347eecce3e712745e23",
    ("o012_apm", "kept"): "c8682ff6107685b760164d0f964ad04b167f17357e180111b953d70b308e8bf7",
    ("o012_apm", "ends"): "8fa786d89bd9a1d59f4fd457ea1e09eb21a938d7f34612833d2385846cc449df",
    ("apm_chain4", "coverage"): "58106febdc9ebffaca225ba3128e6f015b5973f4a01bb557a3a14e0afc4a7d09",
    ("apm_chain4", "kept"): "c01c4f4ea5ff30070ffa7b1ab929b95a556bcc4a4805bc0a87078e8b4305a94d",
    ("apm_chain4", "ends"): "c247c41559023e84bcf35ab8942027e09fd9c279967e8b824edacaebf04807d3",
    ("slot_mix", "coverage"): "3e412c55becd8279b5b8e6fb9eb74273a179ff63deb32334efa50fd182bb36c3",
    ("slot_mix", "kept"): "e23542000048cbcd12c74700ddd85c58dcb148f23c73df863c77e0c62a2fac68",
    ("slot_mix", "ends"): "0aed8a8e6642f4964d8d1a597da14291a1efba77c930f9c579b6f8a4a73725d1",
    ("full_cm_small_tables", "coverage"): "64cb3a15363d8dac65159ae429ddf3a146cc3f5a6fc697742d280d682e54b6aa",
    ("full_cm_small_tables", "kept"): "ac8bd57c604c96be7d7d07d5e4de653d5a8c993773881035f4617434ff2c3fd3",
    ("full_cm_small_tables", "ends"): "8548b28d03ede4aac7062c2a213aeba0d65a591d48a9431e7c7d026dbf534d46",
    ("aoh", 8, "runs"): "dd87a99defdeb8d465a820f6fb0e6b7d603284f6dc0ad74a87491e65d4c37dc3",
    ("aoh", 8, "hold"): "b6cc9d1b9478707ae14ac79a2f263ed88a172f56a74f2d85f071dcd7f0cfb7f7",
    ("aoh", 16, "runs"): "bbbea2ebdf6e20f154975beccafa4a3dd7183b9da51014edf12b6da5bc67f585",
    ("aoh", 16, "hold"): "2f180b8af2633249e66af3f142d9828a33e21584315bedfaba260a22ec0b25f8",
    ("aoh", 25, "runs"): "a84878ce94b4eedfbb8a9de36439df8304cd4f923ccad28531db93323ea5d4d5",
    ("aoh", 25, "hold"): "08ec790e1d7bcc215ae68027c4f66b0b4e490523f1a1b27ad2b05318b33bb576",
}


def counter(name, kind):
    return steer.counter_input(name, counter_pair(orc, name)[1], kind)


def cm(name, kind):
    return steer.cm_input(name, cm_pair(orc, name)[1], kind)


def assert_run_lengths(tr):
    """every exact run length 1..80, and 127 / 128 / 129, 255 / 256 / 257, 1,000 and 4,096 within 2, with first bit 0 and with first bit 1"""
    for first_bit in (0, 1):
        have = tr.run_lengths(first_bit)
        assert [n for n in range(1, 81) if n not in have] == [], first_bit
        for n in (127, 128, 129, 255, 256, 257, 1000, 4096):
            assert have & set(range(n - 2, n + 3)), (n, first_bit)


def assert_single_run(tr):
    """block 0 is ONE run of more than 65,535 bits that only the flush resolves"""
    assert tr.runs[0] == [] and tr.end_pending[0] == tr.longest[0] > 65535, (tr.runs[0][:4], tr.end_pending[0], tr.longest[0])
    assert tr.nblocks == 2 and tr.handback == [True, True]


def assert_block_ends(data, tr, nblocks):
    assert tr.block_size == 48 and tr.nblocks == nblocks >= 192 and len(data) == 48 * nblocks
    seen = collections.Counter(tr.end_pending)
    assert [v for v in range(91) if not seen[v]] == []


def assert_round_trip(factory, data, tr):
    """the trace's streams are those of the oracle's block driver, and its decoder gives the input back"""
    bs = tr.block_size
    out, lens = orc.encode_blocks(factory(), data, bs)
    assert lens.tolist() == tr.lens() and out.tobytes() == tr.stream()
    model = factory()
    for k, s in enumerate(tr.streams):
        blk = data[k * bs:(k + 1) * bs]
        model.reset()
        assert orc.decode_stream(model, s, len(blk)) == blk, k


def assert_digest(key, data):
    assert hashlib.sha256(data).hexdigest() == SHA256[key], key


# ---- Counter models ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_counter_run_lengths(name):
    data, tr = counter(name, "coverage")
    assert tr.block_size == 8192 and len(data) <= 65536
    assert_run_lengths(tr)


@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_counter_kept_runs(name):
    """The run-coverage input is one block, which a fast coder hands back at its first long run: there its short runs reach k_coder
    only.  This input has every run length 1..37 with both first bits in blocks where at most 38 bits are ever pending — fewer than the 39
    pending ones a hand-back needs (w3_coder.h's guard: nb < pend + 8 after the drain, gives up iff nb > 46) — so the carries through
    18 and more ones and the 32-bit moves beside 32 and more pending ones are the fast coders' own."""
    data, tr = counter(name, "kept")
    assert tr.block_size == 128 and tr.nblocks >= 4
    assert max(tr.longest) <= 38 and max(tr.longest) >= 37
    for first_bit in (0, 1):
        assert [n for n in range(1, 38) if n not in tr.run_lengths(first_bit)] == [], first_bit


@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_counter_single_run_over_65535_bits(name):
    data, tr = counter(name, "hold")
    assert tr.block_size == 16384 and 16384 < len(data) < 2 * 16384      # the second block is ragged
    assert_single_run(tr)


@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_counter_block_ends(name):
    data, tr = counter(name, "ends")
    assert_block_ends(data, tr, 192)


@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_counter_mixed(name):
    data, tr = counter(name, "mixed")
    assert tr.block_size == 512 and tr.nblocks == 130 and len(data) == 129 * 512 + 200      # the last block is ragged
    for k in range(130):
        if k % 3 == 0:
            # a run of 64 or more bits followed by more steps: a step coded with 64 or more bits pending
            assert tr.handback[k] and tr.longest[k] >= 64, k
        else:
            assert tr.longest[k] <= 30 and not tr.handback[k], (k, tr.longest[k])
    # the bounds of n_recoded_blocks in tests/test_gpu_steer.py meet: what must be handed back is all that may be
    assert sum(tr.handback) == sum(1 for v in tr.longest if v >= 39) == 44


@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_counter_anti_expands_every_block(name):
    data, tr = counter(name, "anti")
    assert tr.nblocks == 5 and len(data) % tr.block_size
    for k, s in enumerate(tr.streams):
        assert len(s) > len(data[k * tr.block_size:(k + 1) * tr.block_size]), k


@pytest.mark.parametrize("kind", COUNTER_KINDS)
@pytest.mark.parametrize("name", steer.COUNTER_MODELS)
def test_counter_round_trip_and_digest(name, kind):
    data, tr = counter(name, kind)
    assert tr.block_size == steer.BLOCK_SIZE[kind]
    assert_round_trip(counter_pair(orc, name)[1], data, tr)
    assert_digest((name, kind), data)


# ---- CM models -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", steer.CM_MODELS)
def test_cm_run_lengths(name):
    data, tr = cm(name, "coverage")
    assert tr.block_size == 8192 and len(data) <= 65536
    assert_run_lengths(tr)


@pytest.mark.parametrize("name", steer.CM_MODELS)
def test_cm_kept_runs(name):
    data, tr = cm(name, "kept")
    assert tr.block_size == 128 and tr.nblocks >= 4 and 37 <= max(tr.longest) <= 38
    for first_bit in (0, 1):
        assert [n for n in range(1, 38) if n not in tr.run_lengths(first_bit)] == [], first_bit


@pytest.mark.parametrize("name", steer.CM_MODELS)
def test_cm_block_ends(name):
    data, tr = cm(name, "ends")
    assert_block_ends(data, tr, 200)


@pytest.mark.parametrize("kind", CM_KINDS)
@pytest.mark.parametrize("name", steer.CM_MODELS)
def test_cm_round_trip_and_digest(name, kind):
    data, tr = cm(name, kind)
    assert_round_trip(cm_pair(orc, name)[1], data, tr)
    assert_digest((name, kind), data)


# ---- AC over Huffman --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("aoh_ref_steer")


def test_aoh_table_is_complete():
    codes, lens = steer.aoh_table()
    assert max(lens) == steer.AOH_HSIZE and sum(2.0 ** -n for n in lens if n) == 1.0


@pytest.mark.parametrize("cb", steer.AOH_CTX_BITS)
def test_aoh_run_lengths(cb):
    data, tr = steer.aoh_input(cb, "runs")
    assert tr.block_size == 4096 and len(data) <= 65536
    assert_run_lengths(tr)


@pytest.mark.parametrize("cb", steer.AOH_CTX_BITS)
def test_aoh_single_run_over_65535_bits(cb):
    data, tr = steer.aoh_input(cb, "hold")
    bs = steer.AOH_BLOCK_SIZE["hold"]
    assert tr.block_size == bs and bs < len(data) < 2 * bs <= 65536
    assert_single_run(tr)


@pytest.mark.parametrize("kind", AOH_KINDS)
@pytest.mark.parametrize("cb", steer.AOH_CTX_BITS)
def test_aoh_stepping_is_the_drivers_loop(build_dir, cb, kind):
    """the OrderN(ctx_bits, 0) steps through ArithmeticCoder and ACWriter give, byte for byte, the streams of tests/aoh_ref.encode_blocks;
    its decoder gives the input back"""
    data, tr = steer.aoh_input(cb, kind)
    codes, lens = steer.aoh_table()
    bs = tr.block_size
    want, wlens = aoh_ref.encode_blocks(orc, build_dir, codes, lens, cb, data, bs)
    assert wlens.tolist() == tr.lens() and want == tr.stream()
    assert aoh_ref.decode_blocks(orc, build_dir, codes, lens, cb, want, wlens, bs, len(data)) == data
    assert_digest(("aoh", cb, kind), data)
