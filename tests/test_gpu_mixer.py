"""The logistic mixer node (W3_NODE_MIX) on the GPU against tests/mixer_ref.py, the CPU restatement: the two-phase stage (k_lmix /
k_lmix_one, csrc/w3_lmix.h) and the lane kernels (k_cm / k_cm_staged with the mixer flag, csrc/w3_cm.h) — two device implementations of
the encode that must give the reference's bytes and each other's — the decoders on the reference's streams, predictions and bit counts,
the recode path, the injected LDS fault, the pipelined forms, the spec rules and the refusals.  Blocks are at most 4 KiB."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests import apm_census as ac
from tests import mixer_ref as mr
from tests.synth import lcg_text, markov_text
from weath3rb0i_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L2 = mr.DIRECTED_LEAVES
L3 = (("o0",), ("o1",), ("on", 27, 3))
L8 = (("o0",), ("o1",), ("on", 27, 3), ("on", 8, 3), ("ac", 11, 3, 8), ("on", 14, 4), ("on", 5, 3), ("on", 22, 2))   # time-ordered, sorted and wave-per-block leaves
L7S = (("o0",), ("o1",), ("on", 27, 3), ("slot", 1, 10), ("slot", 2, 10), ("slot", 3, 10), ("slot", 4, 10))
A0, A1 = (ac.ORDER0, 7), (ac.ORDER1, 6)
TEXT = markov_text(6000, seed=23) + lcg_text(1200, seed=5) + bytes(300) + b"\xff" * 300

# name: (leaves, selector, rate, APM chain, data, block size) -> block counts 1, 2, 8, 9, 65; block sizes 1, 7, 9, 512, 4096; ragged last blocks
CASES = {
    "n2_order0_r4_zeros_then_ff00": (L2, mr.ORDER0, 4, (), mr.DIRECTED["zeros_then_ff00"], 4096),
    "n2_order0_r4_runs_00_ff": (L2, mr.ORDER0, 4, (), mr.DIRECTED["runs_00_ff"], 4096),
    "n2_one_r4_runs_00_ff": (L2, mr.ONE, 4, (), mr.DIRECTED["runs_00_ff"], 4096),
    "n2_order0_r4_zeros_ones": (L2, mr.ORDER0, 4, (A0,), mr.DIRECTED["zeros"][:2048] + mr.DIRECTED["ones"][:2048], 2048),
    "n2_order0_r4_ramp_ragged": (L2, mr.ORDER0, 4, (), mr.DIRECTED["ramp"] + bytes(range(200)), 512),
    "n3_order0_r14_8_blocks": (L3, mr.ORDER0, 14, (), TEXT[:4096], 512),
    "n3_one_r20_apm0_9_blocks_of_7": (L3, mr.ONE, 20, (A0,), TEXT[100:100 + 7 * 8 + 3], 7),
    "n3_order0_r20_apm1_65_blocks_of_9": (L3, mr.ORDER0, 20, (A1,), TEXT[:9 * 64 + 5], 9),
    "n3_order0_r14_9_blocks_of_1": (L3, mr.ORDER0, 14, (), TEXT[:9], 1),
    "n8_order0_r14_apm01_ragged": (L8, mr.ORDER0, 14, (A0, A1), TEXT[:4096 + 1000], 4096),
    "n8_one_r4_65_blocks_of_1": (L8, mr.ONE, 4, (), TEXT[300:365], 1),
    "n8_order0_r20_apm0_9_blocks": (L8, mr.ORDER0, 20, (A0,), TEXT[2000:2000 + 8 * 300 + 77], 300),
    "n7_slots_order0_r14_apm01": (L7S, mr.ORDER0, 14, (A0, A1), TEXT[:4096 + 333], 4096),
    "n7_slots_one_r14_9_blocks_of_9": (L7S, mr.ONE, 14, (A1,), TEXT[500:500 + 8 * 9 + 2], 9),
}

_REF = {}


def ref(oracle, name):
    """(streams, block lengths, ACStats bits) of the case from the CPU restatement, computed once"""
    if name not in _REF:
        leaves, select, rate, stages, data, bs = CASES[name]
        _REF[name] = mr.encode_blocks(oracle, leaves, data, bs, select, rate, stages)
    return _REF[name]


def model_of(name):
    leaves, select, rate, stages, _, _ = CASES[name]
    return mr.w3_model(w3, leaves, select, rate, stages)


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


def encode(ctx, model, data, bs, path):
    ctx.set_path(path)
    try:
        out, lens = ctx.encode_blocks(model, data, bs)
        return out.tobytes(), lens.tolist(), ctx.timing()
    finally:
        ctx.set_path("auto")


@pytest.mark.parametrize("name", sorted(CASES))
def test_encode_parity_on_both_paths_and_decode(ctx, oracle, name):
    _, _, _, _, data, bs = CASES[name]
    want, wlens, _ = ref(oracle, name)
    two, tlens, tm2 = encode(ctx, model_of(name), data, bs, "twophase")
    lane, llens, tm1 = encode(ctx, model_of(name), data, bs, "generic")
    assert tm2["path"] == L.W3_PATH_TWOPHASE and tm1["path"] == L.W3_PATH_GENERIC
    assert tlens == wlens and two == want, "two-phase stage"
    assert llens == wlens and lane == want, "lane kernel"
    assert two == lane
    auto, alens, _ = encode(ctx, model_of(name), data, bs, "auto")
    assert alens == wlens and auto == want
    # the decoder on the REFERENCE's streams
    back = ctx.decode_blocks(model_of(name), np.frombuffer(want, dtype=np.uint8), np.array(wlens, dtype=np.uint32), bs, len(data))
    assert back.tobytes() == data


@pytest.mark.parametrize("name", ["n3_order0_r20_apm1_65_blocks_of_9", "n8_order0_r14_apm01_ragged", "n7_slots_one_r14_9_blocks_of_9", "n2_one_r4_runs_00_ff"])
def test_predictions_and_bit_counts(ctx, oracle, name):
    leaves, select, rate, stages, data, bs = CASES[name]
    got = ctx.predict_blocks(model_of(name), data, bs)
    assert got.tolist() == mr.predict_blocks(oracle, leaves, data, bs, select, rate, stages)
    for path in ("twophase", "generic"):
        ctx.set_path(path)
        try:
            bits = ctx.encode_stats(model_of(name), data, bs)
        finally:
            ctx.set_path("auto")
        assert bits.tolist() == ref(oracle, name)[2], path


def test_recode_path_keeps_the_mixers_stream(ctx, oracle):
    """blocks the fast coder hands back are recoded from ws.P: the mixer's stream, not an OpinionMixer2 merge of the leaves.  On text
    with W3_OPT_ACC_LIMIT = 19: blocks are handed back and the output is what it is without the limit and what the lane kernel writes
    (both equal to the restatement in the parity cases above)."""
    data = markov_text(256 * 1024 + 77, seed=61) + lcg_text(64 * 1024, seed=8)
    for model in (mr.w3_model(w3, L3, mr.ORDER0, 14), mr.w3_model(w3, L3, mr.ONE, 16, (A0, A1))):
        plain = encode(ctx, model, data, 4096, "twophase")
        lane = encode(ctx, model, data, 4096, "generic")
        assert plain[2]["n_recoded_blocks"] == 0 and plain[:2] == lane[:2]
        ctx.set_acc_limit(19)
        try:
            out, lens, tm = encode(ctx, model, data, 4096, "twophase")
        finally:
            ctx.set_acc_limit(46)
        print("recoded blocks:", tm["n_recoded_blocks"])
        assert tm["n_recoded_blocks"] > 0
        assert (out, lens) == plain[:2]


def test_a_block_held_in_one_pending_run_is_handed_back_and_recoded(ctx, oracle):
    """a block steered so that every bit keeps the coder astride the midpoint under the MIXER's predictions: no fast coder can hold the
    run (64 pending bits and more), so the block goes through the recode path at the default limit — against the restatement"""
    held, longest = mr.held_block(oracle, L3, 300, mr.ORDER0, 14, (A0,))
    assert longest >= 64
    data = held + TEXT[:212]
    want, wlens, _ = mr.encode_blocks(oracle, L3, data, 512, mr.ORDER0, 14, (A0,))
    out, lens, tm = encode(ctx, mr.w3_model(w3, L3, mr.ORDER0, 14, (A0,)), data, 512, "twophase")
    assert tm["n_recoded_blocks"] == 1
    assert lens == wlens and out == want


def test_auto_takes_the_measured_path(ctx):
    """W3_PATH_AUTO: the two-phase stage from the size and block size it was measured to win at (99,942,400 bytes in 64 KiB blocks:
    profiles/mixer/), the lane kernel everywhere else; the two-phase call asked for by name writes the same bytes"""
    m = w3.order012_mix()
    big = np.frombuffer(TEXT, dtype=np.uint8)
    big = np.tile(big, 99942400 // len(big) + 1)[:99942400]
    out, lens = ctx.encode_blocks(m, big, 65536)
    assert ctx.timing()["path"] == L.W3_PATH_TWOPHASE
    ctx.set_path("twophase")
    try:
        out2, lens2 = ctx.encode_blocks(m, big, 65536)
    finally:
        ctx.set_path("auto")
    assert lens.tolist() == lens2.tolist() and np.array_equal(out, out2)
    for n, bs in ((65536, 4096), (99942400 - 65536, 65536)):   # blocks smaller than the measured ones; an input below the measured size
        if n > 65536:   # (the lane kernel at that size takes seconds: the rule's answer alone)
            continue
        _, _, tm = encode(ctx, m, big[:n], bs, "auto")
        assert tm["path"] == L.W3_PATH_GENERIC, (n, bs)


def test_injected_lds_fault_is_caught_and_the_output_unchanged(oracle):
    name = "n3_order0_r14_8_blocks"
    _, _, _, _, data, bs = CASES[name]
    want, wlens, _ = ref(oracle, name)
    c = w3.Context(0)
    try:
        c.set_variant("inject_lds_fault")
        out, lens, tm = encode(c, model_of(name), data, bs, "twophase")
        assert tm["n_lds_faults"] > 0
        assert lens == wlens and out == want
        out, lens, tm = encode(c, model_of(name), data, bs, "twophase")   # the context stays on the ballot path
        assert tm["n_lds_faults"] == 0 and lens == wlens and out == want
    finally:
        c.close()


def test_decode_ranges_checked_and_unstaged(ctx, oracle):
    name = "n7_slots_order0_r14_apm01"
    _, _, _, _, data, bs = CASES[name]
    want, wlens, _ = ref(oracle, name)
    comp, lens = np.frombuffer(want, dtype=np.uint8), np.array(wlens, dtype=np.uint32)
    ranges = [(4090, 20), (0, 1), (4200, len(data) - 4200)]
    got = ctx.decode_ranges(model_of(name), comp, lens, bs, len(data), ranges)
    assert got.tobytes() == b"".join(data[o:o + n] for o, n in ranges)
    crc = ctx.crc32_blocks(data, bs)
    assert ctx.decode_blocks(model_of(name), comp, lens, bs, len(data), crc=crc).tobytes() == data
    bad = crc.copy()
    bad[1] ^= 1
    with pytest.raises(w3.W3Error) as e:
        ctx.decode_blocks(model_of(name), comp, lens, bs, len(data), crc=bad)
    assert e.value.code == L.W3_E_CORRUPT and e.value.bad_block == 1
    ctx.set_variant("cm_unstaged")
    try:
        assert ctx.decode_blocks(model_of(name), comp, lens, bs, len(data)).tobytes() == data
        lane, llens, _ = encode(ctx, model_of(name), data, bs, "generic")
        assert llens == wlens and lane == want
    finally:
        ctx.set_variant()


def test_two_submitted_jobs_in_flight_equal_the_synchronous_call(oracle):
    import torch
    names = ["n8_order0_r14_apm01_ragged", "n3_order0_r14_8_blocks"]
    c = w3.Context(0)
    try:
        c.set_path("twophase")
        d_ins = [torch.from_numpy(np.frombuffer(CASES[nm][4], dtype=np.uint8).copy()).cuda() for nm in names]
        bufs = [(torch.empty(2 * len(CASES[nm][4]) + 4096, dtype=torch.uint8, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda"),
                 torch.zeros(1, dtype=torch.int64, device="cuda")) for nm in names]
        torch.cuda.synchronize()
        for rnd in range(2):
            jobs = [c.encode_submit(model_of(nm), d_ins[k], CASES[nm][5], *bufs[k]) for k, nm in enumerate(names)]
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
    names = ["n7_slots_order0_r14_apm01", "n3_order0_r20_apm1_65_blocks_of_9"]
    c = w3.Context(0)
    try:
        c.set_path("twophase")
        ins = [np.frombuffer(CASES[nm][4], dtype=np.uint8).copy() for nm in names]
        outs = [(np.zeros(2 * len(CASES[nm][4]) + 8192, dtype=np.uint8), np.zeros(128, dtype=np.uint32)) for nm in names]
        jobs = [c.encode_host_submit(model_of(nm), ins[k], CASES[nm][5], *outs[k]) for k, nm in enumerate(names)]
        for k, nm in enumerate(names):
            total = c.encode_host_wait(jobs[k])
            want, wlens, _ = ref(oracle, nm)
            assert total == len(want) and outs[k][1][:len(wlens)].tolist() == wlens and outs[k][0][:total].tobytes() == want, nm
    finally:
        c.close()


def _spec(*nodes):
    s = L.ModelSpec()
    s.n_nodes = len(nodes)
    for i, (kind, bits, align, max_bits, extra) in enumerate(nodes):
        nd = L.Node()
        nd.kind, nd.bits, nd.align, nd.max_bits = kind, bits, align, max_bits
        for k, v in extra.items():
            setattr(nd, k, v)
        s.nodes[i] = nd
    return L.load().w3_spec_validate(C.byref(s))


def test_spec_rules():
    O0, O1 = (L.W3_NODE_ORDERN, 11, 3, 0, {}), (L.W3_NODE_ORDERN, 19, 3, 0, {})
    SL = (L.W3_NODE_SLOT_STATE, 2, 0, 0, {"log_cells": 10})
    BO2, APM = (L.W3_NODE_BEST_OF_TWO, 0, 0, 0, {}), (L.W3_NODE_APM, 0, 0, 7, {})

    def MIX(n=2, sel=L.W3_MIX_ORDER0, rate=14, **extra):
        return (L.W3_NODE_MIX, n, sel, rate, extra)
    assert _spec(O0, O1, MIX()) == 0 and _spec(O0, SL, MIX(), APM, APM) == 0 and _spec(*([O0] * 8), MIX(8, L.W3_MIX_ONE, 4)) == 0
    assert _spec(O0, O1, MIX(rate=20)) == 0
    # bad field values, nothing to pop
    for bad in (MIX(1), MIX(9), MIX(0), MIX(sel=2), MIX(rate=3), MIX(rate=21), MIX(history=1), MIX(frozen=1), MIX(log_cells=1), MIX(reserved=1)):
        assert _spec(O0, O1, bad) == L.W3_E_INVALID, bad
    assert _spec(O0, MIX()) == L.W3_E_INVALID and _spec(MIX()) == L.W3_E_INVALID and _spec(O0, O1, MIX(3)) == L.W3_E_INVALID
    # valid shapes that are not built
    FRO = (L.W3_NODE_ORDERN, 19, 3, 0, {"frozen": 1})
    assert _spec(O0, O1, BO2, O1, MIX()) == L.W3_E_UNSUPPORTED          # a BestOfTwo under it
    assert _spec(O0, FRO, MIX()) == L.W3_E_UNSUPPORTED                  # a frozen leaf under it
    assert _spec(O0, O0, O1, MIX()) == L.W3_E_UNSUPPORTED               # a leaf beside it
    assert _spec(O0, O1, MIX(), O0, BO2) == L.W3_E_UNSUPPORTED          # a leaf beside it, after it
    assert _spec(O0, O1, MIX(), O0, MIX()) == L.W3_E_UNSUPPORTED        # a second mixer
    assert _spec(O0, O1, MIX(), MIX()) == L.W3_E_UNSUPPORTED
    assert _spec(O0, APM, O1, MIX()) == L.W3_E_UNSUPPORTED              # a mixer after an APM
    assert _spec(O0, APM, MIX()) == L.W3_E_UNSUPPORTED
    # the Python mirror
    assert w3.order012_mix().spec().n_nodes == 4 and w3.full_cm_mix().spec().n_nodes == 10
    for m, code in ((w3.LogisticMixer([w3.Order0()]), L.W3_E_INVALID), (w3.LogisticMixer([w3.Order0(), w3.FrozenModel(w3.Order1())]), L.W3_E_UNSUPPORTED),
                    (w3.LogisticMixer([w3.Order0(), w3.Order1()], rate=3), L.W3_E_INVALID), (w3.BestOfTwoModel(w3.order012_mix(), w3.Order0()), L.W3_E_UNSUPPORTED)):
        with pytest.raises(w3.W3Error) as e:
            m.spec()
        assert e.value.code == code
    assert L.load().w3_abi_version() == 8 and C.sizeof(L.Node) == 24


def test_what_is_not_built_is_refused(ctx):
    import torch
    m = w3.order012_mix()
    with pytest.raises(w3.W3Error) as e:
        w3.Context.steps_layout(m)
    assert e.value.code == L.W3_E_UNSUPPORTED
    spec = m.spec()
    data = np.frombuffer(TEXT[:1024], dtype=np.uint8).copy()
    rows = np.zeros(8 * 1024 * 8, dtype=np.uint16)
    rc = ctx.lib.w3_export_steps_staged(ctx.h, C.byref(spec), data.ctypes.data_as(C.c_void_p), len(data), 512, L.W3_STEPS_P_U16, 0,
                                        rows.ctypes.data_as(C.c_void_p), rows.nbytes)
    assert rc == L.W3_E_UNSUPPORTED and b"W3_NODE_MIX" in ctx.lib.w3_last_error(ctx.h)
    d_in = torch.from_numpy(data).cuda()
    d_rows = torch.zeros(8 * 1024 * 8, dtype=torch.int16, device="cuda")
    rc = ctx.lib.w3_export_steps_device(ctx.h, C.byref(spec), C.c_void_p(d_in.data_ptr()), len(data), 512, L.W3_STEPS_P_U16, 0,
                                        C.c_void_p(d_rows.data_ptr()), d_rows.numel() * 2, None)
    assert rc == L.W3_E_UNSUPPORTED
    for export in (ctx.export_counters, ctx.export_counters_staged, ctx.export_entropy_staged):   # the single-leaf exports
        with pytest.raises(w3.W3Error) as e:
            export(m, TEXT[:1024])
        assert e.value.code == L.W3_E_UNSUPPORTED, export
    # a block size outside the predict kernels' cover: the stage is refused by name, the lane kernel codes it
    ctx.set_path("twophase")
    try:
        with pytest.raises(w3.W3Error) as e:
            ctx.encode_blocks(m, TEXT[:5], 4)
        assert e.value.code == L.W3_E_UNSUPPORTED
    finally:
        ctx.set_path("auto")


def test_cli_round_trips_a_small_file(tmp_path):
    cli = os.path.join(ROOT, "tools", "w3")
    src = os.path.join(ROOT, "tools", "w3cli.cpp")
    if not os.path.exists(cli) or os.path.getmtime(cli) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", cli, src, "-L" + os.path.join(ROOT, "weath3rb0i_amd"), "-lw3hip",
                               "-Wl,-rpath,$ORIGIN/../weath3rb0i_amd", "-Wl,-rpath,/opt/rocm/lib"])
    data = TEXT[:5000]
    f = tmp_path / "small.txt"
    f.write_bytes(data)
    e = dict(os.environ, W3_MODEL="order012mix")
    r = subprocess.run([cli, "t", str(f)], cwd=tmp_path, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "small.orig").read_bytes() == data
    blob = (tmp_path / "small.bin").read_bytes()
    assert blob[:4] == b"w3bk"
    c = w3.Context(0)
    try:
        out, lens = c.encode_blocks(w3.order012_mix(), data, 65536)
    finally:
        c.close()
    assert blob.endswith(out.tobytes()) and len(out) < len(data) // 2
