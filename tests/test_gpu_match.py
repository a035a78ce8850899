"""The match-model leaf (W3_HIST_MATCH) on the GPU against tests/match_ref.py, the CPU restatement: the two-phase key stage (k_match_keys,
csrc/w3_match.h, feeding k_predict_small) and the lane kernels with the MATCH flag (k_generic, k_cm_staged, k_cm: csrc/w3_generic.h,
w3_cm.h) — two device implementations that must give the restatement's predictions, bytes and bit counts — the decoders on the
restatement's streams, ranges, a checked decode, the container, the pipelined forms, the injected LDS fault, the step rows, the refusals and
the CLI.  Blocks are at most 4 KiB."""
import os
import subprocess

import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests import apm_census as ac
from tests import match_ref as mt
from tests import mixer_ref as mr
from weath3rb0i_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A0, A1 = (ac.ORDER0, 7), (ac.ORDER1, 6)
TEXT = mt.DIRECTED["phrases"][:2600] + mt.DIRECTED["nibbles"][:900] + bytes(300) + b"\xff" * 100 + mt.DIRECTED["bytes"][:700] + mt.DIRECTED["pairs"][:600]


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


# ---- (a) the single leaf's predictions --------------------------------------------------------------------------------------------------
# name: (data, block size, (m, L)).  Directed inputs as one block each, the three configurations in turn; random and text bytes in blocks
# of 1, 3, 7, 8, 63, 64, 65, 200 and 4096 with a ragged last block, 1, 5 and 65 blocks.
LEAF_CASES = {"directed_" + nm: (mt.DIRECTED[nm], 4096, mt.CONFIGS[k % 3]) for k, nm in enumerate(sorted(mt.DIRECTED))}
LEAF_CASES.update({
    "zeros_2_8": (mt.DIRECTED["zeros"], 4096, (2, 8)),
    "zeros_3_12": (mt.DIRECTED["zeros"], 4096, (3, 12)),
    "bytes_65_blocks_of_1": (mt.DIRECTED["bytes"][:65], 1, (2, 8)),
    "pairs_5_blocks_of_3": (mt.DIRECTED["pairs"][:3 * 4 + 2], 3, (2, 8)),
    "pairs_65_blocks_of_7": (mt.DIRECTED["pairs"][:7 * 64 + 3], 7, (2, 8)),
    "pairs_5_blocks_of_8": (mt.DIRECTED["pairs"][100:100 + 8 * 4 + 5], 8, (3, 12)),
    "text_5_blocks_of_63": (TEXT[:63 * 4 + 10], 63, (4, 16)),
    "text_65_blocks_of_64": (TEXT[:64 * 64 + 1], 64, (4, 16)),
    "nibbles_5_blocks_of_65": (mt.DIRECTED["nibbles"][:65 * 4 + 64], 65, (2, 8)),
    "bytes_5_blocks_of_200": (mt.DIRECTED["bytes"][:200 * 4 + 77], 200, (2, 8)),
    "text_ragged_4096": (TEXT[:4096 + 1000], 4096, (3, 12)),
    "bytes_one_block_l20": (mt.DIRECTED["bytes"], 4096, (4, 20)),
})


@pytest.mark.parametrize("name", sorted(LEAF_CASES))
def test_the_leafs_predictions(ctx, oracle, name):
    data, bs, (m, Ls) = LEAF_CASES[name]
    leaves = (("match", m, Ls),)
    want = mt.predict_blocks(oracle, leaves, data, bs, "leaf")
    ctx.set_path("twophase")
    try:
        got = ctx.predict_blocks(w3.MatchModel(m, Ls), data, bs)
    finally:
        ctx.set_path("auto")
    assert got.tolist() == want


# ---- (b) whole models on both paths -------------------------------------------------------------------------------------------------------
# name: (leaves, combine, APM chain, data, block size, the package's model)
MODEL_CASES = {
    "order012_match_mix": (mt.O012M, "mix", (), TEXT[:4096 + 700], 2048, w3.order012_match_mix),
    "tree_o0_match_o1": ((("o0",), ("match", 3, 12), ("o1",)), "tree", (), TEXT[1000:1000 + 2 * 1500 + 99], 1500,
                         lambda: w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.MatchModel(3, 12)), w3.Order1())),
    "leaf_apm01": ((("match", 4, 16),), "leaf", (A0, A1), TEXT[:2 * 1200 + 300], 1200,
                   lambda: w3.APM(w3.APM(w3.MatchModel(), w3.APM.ORDER0, 7), w3.APM.ORDER1, 6)),
    "full_cm_match_mix_8": (mt.full_cm_leaves(8), "mix", (A0, A1), TEXT[500:500 + 2 * 1024 + 200], 1024, lambda: w3.full_cm_match_mix(log_cells=8)),
    "match_mix_65_blocks_of_9": ((("o0",), ("match", 2, 8)), "mix", (A0,), mt.DIRECTED["pairs"][:9 * 64 + 5], 9,
                                 lambda: w3.APM(w3.LogisticMixer([w3.Order0(), w3.MatchModel(2, 8)]), w3.APM.ORDER0, 7)),
}
_REF = {}


def ref(oracle, name):
    """(streams, block lengths, ACStats bits) of the case from the CPU restatement, computed once"""
    if name not in _REF:
        leaves, combine, stages, data, bs, _ = MODEL_CASES[name]
        _REF[name] = mt.encode_blocks(oracle, leaves, data, bs, combine, stages=stages)
    return _REF[name]


def encode(ctx, model, data, bs, path):
    ctx.set_path(path)
    try:
        out, lens = ctx.encode_blocks(model, data, bs)
        return out.tobytes(), lens.tolist(), ctx.timing()
    finally:
        ctx.set_path("auto")


@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_encode_bytes_and_bit_counts_on_both_paths(ctx, oracle, name):
    _, _, _, data, bs, model = MODEL_CASES[name]
    want, wlens, wbits = ref(oracle, name)
    two, tlens, tm2 = encode(ctx, model(), data, bs, "twophase")
    lane, llens, tm1 = encode(ctx, model(), data, bs, "generic")
    assert tm2["path"] == L.W3_PATH_TWOPHASE and tm1["path"] == L.W3_PATH_GENERIC
    assert tlens == wlens and two == want, "two-phase path"
    assert llens == wlens and lane == want, "lane kernel"
    for path in ("twophase", "generic"):
        ctx.set_path(path)
        try:
            bits = ctx.encode_stats(model(), data, bs)
        finally:
            ctx.set_path("auto")
        assert bits.tolist() == wbits, path


def test_the_key_stage_is_timed(ctx):
    ctx.set_timing(True)
    try:
        _, _, tm = encode(ctx, w3.order012_match_mix(), TEXT, 2048, "twophase")
        assert 0.0 < tm["match_ms"] <= tm["predict_ms"]
        _, _, tm = encode(ctx, w3.order012_mix(), TEXT, 2048, "twophase")
        assert tm["match_ms"] == 0.0
    finally:
        ctx.set_timing(False)


# ---- (c) decode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("tree_o0_match_o1", ()), ("order012_match_mix", ()), ("leaf_apm01", ()), ("full_cm_match_mix_8", ()),
                                          ("match_mix_65_blocks_of_9", ()), ("full_cm_match_mix_8", ("cm_unstaged",)), ("leaf_apm01", ("cm_unstaged",))])
def test_the_lane_kernels_decode_the_restatements_streams(ctx, oracle, name, variant):
    """k_generic (the tree without stages), k_cm_staged (a mixer or APM stages), k_cm (the unstaged variant)"""
    _, _, _, data, bs, model = MODEL_CASES[name]
    want, wlens, _ = ref(oracle, name)
    assert not w3.Context.decode_spec_covers(model())
    ctx.set_variant(*variant)
    try:
        back = ctx.decode_blocks(model(), np.frombuffer(want, dtype=np.uint8), np.array(wlens, dtype=np.uint32), bs, len(data))
        assert ctx.last_decode_path() == L.W3_PATH_GENERIC
        assert back.tobytes() == data
        if variant:
            lane, llens, _ = encode(ctx, model(), data, bs, "generic")
            assert llens == wlens and lane == want
    finally:
        ctx.set_variant()


@pytest.mark.parametrize("name", ["order012_match_mix", "tree_o0_match_o1"])
def test_ranges_checked_decode_and_container(ctx, oracle, name):
    _, _, _, data, bs, model = MODEL_CASES[name]
    want, wlens, _ = ref(oracle, name)
    comp, lens = np.frombuffer(want, dtype=np.uint8), np.array(wlens, dtype=np.uint32)
    ranges = [(bs - 6, 20), (0, 1), (bs + 100, len(data) - bs - 100), (5, 700)]
    got = ctx.decode_ranges(model(), comp, lens, bs, len(data), ranges)
    assert got.tobytes() == b"".join(data[o:o + n] for o, n in ranges)
    crc = ctx.crc32_blocks(data, bs)
    assert ctx.decode_blocks(model(), comp, lens, bs, len(data), crc=crc).tobytes() == data
    bad = crc.copy()
    bad[1] ^= 1
    with pytest.raises(w3.W3Error) as e:
        ctx.decode_blocks(model(), comp, lens, bs, len(data), crc=bad)
    assert e.value.code == L.W3_E_CORRUPT and e.value.bad_block == 1
    # the reference container: one stream, one lane
    blob = ctx.compress(data[:1500], model())
    one, _, _ = mt.encode_blocks(oracle, MODEL_CASES[name][0], data[:1500], 1500, MODEL_CASES[name][1])
    assert blob.endswith(one) and ctx.decompress(blob, model()) == data[:1500]


# ---- (d) the pipelined forms ----------------------------------------------------------------------------------------------------------------
def test_two_submitted_jobs_in_flight_equal_the_synchronous_call(oracle):
    import torch
    names = ["order012_match_mix", "full_cm_match_mix_8"]
    c = w3.Context(0)
    try:
        c.set_path("twophase")
        d_ins = [torch.from_numpy(np.frombuffer(MODEL_CASES[nm][3], dtype=np.uint8).copy()).cuda() for nm in names]
        bufs = [(torch.empty(2 * len(MODEL_CASES[nm][3]) + 4096, dtype=torch.uint8, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda"),
                 torch.zeros(1, dtype=torch.int64, device="cuda")) for nm in names]
        torch.cuda.synchronize()
        for rnd in range(2):
            jobs = [c.encode_submit(MODEL_CASES[nm][5](), d_ins[k], MODEL_CASES[nm][4], *bufs[k]) for k, nm in enumerate(names)]
            for k in (1, 0):
                c.encode_wait(jobs[k])
                assert c.timing()["path"] == L.W3_PATH_TWOPHASE
                want, wlens, _ = ref(oracle, names[k])
                d_out, d_lens, d_total = bufs[k]
                assert d_lens[:len(wlens)].cpu().numpy().astype(np.uint32).tolist() == wlens, (rnd, k)
                assert d_out[: int(d_total.item())].cpu().numpy().tobytes() == want, (rnd, k)
    finally:
        c.close()


def test_host_submit_and_wait_equal_the_synchronous_call(oracle):
    names = ["leaf_apm01", "match_mix_65_blocks_of_9"]
    c = w3.Context(0)
    try:
        c.set_path("twophase")
        ins = [np.frombuffer(MODEL_CASES[nm][3], dtype=np.uint8).copy() for nm in names]
        outs = [(np.zeros(2 * len(MODEL_CASES[nm][3]) + 8192, dtype=np.uint8), np.zeros(128, dtype=np.uint32)) for nm in names]
        jobs = [c.encode_host_submit(MODEL_CASES[nm][5](), ins[k], MODEL_CASES[nm][4], *outs[k]) for k, nm in enumerate(names)]
        for k, nm in enumerate(names):
            total = c.encode_host_wait(jobs[k])
            want, wlens, _ = ref(oracle, nm)
            assert total == len(want) and outs[k][1][:len(wlens)].tolist() == wlens and outs[k][0][:total].tobytes() == want, nm
    finally:
        c.close()


# ---- (e) the injected LDS fault -------------------------------------------------------------------------------------------------------------
def test_injected_lds_fault_is_caught_and_the_output_unchanged(oracle):
    name = "order012_match_mix"
    _, _, _, data, bs, model = MODEL_CASES[name]
    want, wlens, _ = ref(oracle, name)
    c = w3.Context(0)
    try:
        c.set_variant("inject_lds_fault")
        c.set_fault_kernels("predict_small")
        out, lens, tm = encode(c, model(), data, bs, "twophase")
        assert tm["n_lds_faults"] > 0
        assert lens == wlens and out == want
    finally:
        c.close()


# ---- (f) step rows and the refused exports ----------------------------------------------------------------------------------------------------
def test_the_leafs_column_of_the_step_rows_and_the_refused_exports(ctx, oracle):
    data, bs = TEXT[:2 * 1000 + 123], 1000
    leaves = (("o0",), ("match", 3, 12))
    model = w3.BestOfTwoModel(w3.Order0(), w3.MatchModel(3, 12))
    rows = ctx.export_steps(model, data, bs, "p_u16", bit=False)
    lay = ctx.steps_layout(model, "p_u16", False)
    assert lay["n_leaves"] == 2
    want = []
    for blk in mr.blocks_of(data, bs):
        want += mt.leaf_stream(blk, 3, 12)
    assert rows[:, 1].tolist() == want
    assert rows[:, lay["col_final"]].tolist() == mt.predict_blocks(oracle, leaves, data, bs, "tree")
    for export in (ctx.export_counters, ctx.export_counters_staged, ctx.export_entropy_staged):
        with pytest.raises(w3.W3Error) as e:
            export(w3.MatchModel(), TEXT[:1024])
        assert e.value.code == L.W3_E_UNSUPPORTED, export


# ---- (g) the CLI ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", [("order012matchmix", w3.order012_match_mix), ("fullcmmatchmix", w3.full_cm_match_mix)])
def test_cli_round_trips_a_small_file(tmp_path, name, model):
    cli = os.path.join(ROOT, "tools", "w3")
    src = os.path.join(ROOT, "tools", "w3cli.cpp")
    if not os.path.exists(cli) or os.path.getmtime(cli) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", cli, src, "-L" + os.path.join(ROOT, "weath3rb0i_amd"), "-lw3hip",
                               "-Wl,-rpath,$ORIGIN/../weath3rb0i_amd", "-Wl,-rpath,/opt/rocm/lib"])
    data = TEXT[:5000]
    f = tmp_path / "small.txt"
    f.write_bytes(data)
    e = dict(os.environ, W3_MODEL=name)
    r = subprocess.run([cli, "t", str(f)], cwd=tmp_path, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "small.orig").read_bytes() == data
    blob = (tmp_path / "small.bin").read_bytes()
    assert blob[:4] == b"w3bk"
    c = w3.Context(0)
    try:
        out, lens = c.encode_blocks(model(), data, 65536)
    finally:
        c.close()
    assert blob.endswith(out.tobytes()) and len(out) < len(data)
