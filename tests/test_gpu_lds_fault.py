"""The insurance against the one undocumented hardware property the default predict kernels rely on — returning LDS adds of one
wavefront resolve in ascending lane order (k_predict_small's and k_rank_sorted's atomic rounds, k_partition8's cursor adds) — end to end:
  - the fault hook (W3_OPT_VARIANT inject_lds_fault, W3_OPT_FAULT_KERNELS) mis-orders one round of returning adds per block in each of the
    three kernels, and the sampled verification (W3_OPT_VERIFY) catches it;
  - a fault confined to one block is caught within the ceil(nb / S) calls the schedule (csrc/w3_verify.h) promises, whichever block it is;
  - every encode entry point recovers: the faulting call returns the oracle's streams and the context stays on the ballot path;
  - that ballot path (W3_OPT_VARIANT no_lds_atomics: ballot rounds, 4-bit partition passes, k_slot for slot leaves) matches the oracle
    over the models, block sizes and edge cases it has to carry after a fault.
Every stream comparison is byte for byte against oracle.encode_blocks, every predict comparison step for step against oracle.predict_all."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import weath3rb0i_amd as w3
from tests.synth import lcg_text, markov_text
from tests.test_gpu_parity import TWOPHASE, _device_bufs, check_blocks, pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("predict_small", "rank_sorted", "partition8")


_SCHEDULE = {}


def first_sampled(nb, short_last, bs, v, block):
    """The first call (counted from a fresh context's first call of the shape) whose verification sample holds the block: the schedule's
    own functions (w3_verify.h), compiled for the host by the harness of tests/test_verify_schedule.py (built on first use)."""
    if "exe" not in _SCHEDULE:
        exe = os.path.join(tempfile.mkdtemp(prefix="w3vs"), "verify_schedule")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "verify_schedule.cpp")])
        _SCHEDULE["exe"] = exe
    r = subprocess.run([_SCHEDULE["exe"], "first", str(nb), str(int(short_last)), str(bs), str(v), str(block)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return int(r.stdout.strip())


def _faulty_ctx(kernels=KERNELS, block=-1):
    """A context with the fault hook on, in `kernels` (None: the hook's default kernel, k_predict_small), in `block` (-1: every block)."""
    c = w3.Context(0)
    c.set_variant("inject_lds_fault")
    if kernels is not None:
        c.set_fault_kernels(*kernels)
    c.set_fault_block(block)
    return c


def _encode(c, model, data, bs):
    """-> (streams, block lengths, n_lds_faults) of one w3_encode_blocks call"""
    out, lens = c.encode_blocks(model, data, bs)
    return out, lens, c.timing()["n_lds_faults"]


def _caught_at(calls, victim, want):
    """Run `calls` (each -> (streams, block lengths, n_lds_faults)) until the verification reports a fault, at most as many calls as the
    schedule's bound allows (len(calls)); before it the corrupted stream goes out, the faulting call returns the oracle's.
    -> the index of the call that caught it"""
    for k, call in enumerate(calls):
        out, lens, faults = call()
        if faults > 0:
            assert lens.tolist() == want[1].tolist() and out.tobytes() == want[0].tobytes(), (victim, k)   # re-encoded on the ballot path
            return k
        assert out.tobytes() != want[0].tobytes(), (victim, k)   # not sampled yet: the one corrupted block goes out
    raise AssertionError("a fault in block %d was not caught within %d calls" % (victim, len(calls)))


def _runs_where_partition8_is_hooked(data, bs, kernel):
    """For the k_partition8 hook: a run of one byte over positions 56 .. 135 of every block.  The hooked round (round 1 of a block's
    first tile: positions 64 .. 127) lets two records of one bin swap places; that changes a prediction only where the two share their
    Counter keys — records with different keys may be ranked in either order with the same result (and the verification rightly finds
    nothing then).  In a run they share them."""
    if kernel != "partition8":
        return data
    b = bytearray(data)
    for o in range(0, len(b), bs):
        k = len(b[o + 56:o + 136])
        b[o + 56:o + 56 + k] = b"e" * k
    return bytes(b)


def _o012_apm(oracle):
    return (lambda: w3.APM(w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3))),
            lambda: oracle.APM(oracle.BestOfTwoModel(oracle.BestOfTwoModel(oracle.Order0(), oracle.Order1()), oracle.OrderN(27, 3))))


# ---------------------------------------------------------------------------------------------------------------------------------
# C.1 detection in each kernel
# ---------------------------------------------------------------------------------------------------------------------------------
# the models whose leaves reach the kernel (an order-2 leaf alone sorts with the 4-bit passes: k_partition8 runs for Order1-shaped
# leaves and for an order-2 leaf chained behind one)
REACH = [("predict_small", "order0"), ("predict_small", "main_default"), ("rank_sorted", "order1"), ("rank_sorted", "best012"),
         ("rank_sorted", "order2"), ("partition8", "order1"), ("partition8", "best012")]


@pytest.mark.parametrize("kernel,name", REACH)
def test_verification_catches_a_misordered_add_in_each_kernel(oracle, kernel, name):
    bs = 16384
    data = _runs_where_partition8_is_hooked(markov_text(300000, seed=23) + lcg_text(30000, seed=6), bs, kernel)
    dev, orc = pair(oracle, name)
    want, wlens = oracle.encode_blocks(orc(), data, bs, nthreads=8)
    c = w3.Context(0)
    try:
        c.set_path("twophase")
        out, lens = c.encode_blocks(dev(), data, bs)                        # clean run: verification on, nothing found
        assert c.timing()["n_lds_faults"] == 0 and out.tobytes() == want.tobytes()
        c.set_variant("inject_lds_fault")
        c.set_fault_kernels(kernel)
        out, lens = c.encode_blocks(dev(), data, bs)
        assert c.timing()["n_lds_faults"] > 0, (kernel, name)
        assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes(), (kernel, name)   # re-encoded on the ballot path
        out, lens = c.encode_blocks(dev(), data, bs)                        # the context stays there: nothing to find
        assert c.timing()["n_lds_faults"] == 0 and out.tobytes() == want.tobytes(), (kernel, name)
    finally:
        c.close()


@pytest.mark.parametrize("kernel,name", [("predict_small", "order0"), ("rank_sorted", "order1"), ("partition8", "order1")])
def test_fault_hook_changes_the_kernels_output(oracle, kernel, name):
    """predict_blocks has no verification: there the hook's corruption of each kernel shows against oracle.predict_all (the hook
    really changes that kernel's output), and without the hook the same call is exact."""
    bs = 16384
    data = _runs_where_partition8_is_hooked(markov_text(131072, seed=23), bs, kernel)
    dev, orc = pair(oracle, name)
    ref = np.concatenate([oracle.predict_all(orc(), data[o:o + bs]) for o in range(0, len(data), bs)])
    c = w3.Context(0)
    try:
        assert np.array_equal(c.predict_blocks(dev(), data, bs), ref)
        c.set_variant("inject_lds_fault")
        c.set_fault_kernels(kernel)
        assert not np.array_equal(c.predict_blocks(dev(), data, bs), ref), (kernel, name)
        with pytest.raises(w3.W3Error):                                     # the hook cannot be used to corrupt OUTPUT
            c.set_verify(False)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# C.2 every block is reachable
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_fault_in_any_block_is_caught_within_the_bound(oracle):
    """410 full 1 KiB blocks and a 333-byte one: S = 16 does not divide the block count.  The victims: blocks the formula of rounds 1 - 4
    never sampled (s * nb_full / S + (call mod floor(nb_full / S))), the short last block, block 0 and the last full block.  Each is
    caught within ceil(nb / S) calls, at the call the schedule names; the corrupted stream goes out before that call, and from that
    call on the streams are the oracle's."""
    bs, nb_full, tail = 1024, 410, 333
    nb, S = nb_full + 1, 16
    G = -(-nb // S)
    data = markov_text(bs * nb_full + tail, seed=29)
    dev, orc = pair(oracle, "order0")
    want = oracle.encode_blocks(orc(), data, bs, nthreads=8)
    old = {s * nb_full // S + r for r in range(nb_full // S) for s in range(S)}
    unreached = sorted(set(range(nb_full)) - old)
    assert unreached and nb_full - 1 in unreached
    for victim in (unreached[0], unreached[len(unreached) // 2], nb_full - 1, nb_full, 0):
        c = _faulty_ctx(None, victim)
        try:
            c.set_path("twophase")
            caught = _caught_at([lambda: _encode(c, dev(), data, bs)] * G, victim, want)
            assert caught == first_sampled(nb, True, bs, 1, victim), (victim, caught)
            out, lens = c.encode_blocks(dev(), data, bs)
            assert c.timing()["n_lds_faults"] == 0 and out.tobytes() == want[0].tobytes(), victim
        finally:
            c.close()


def test_a_fault_is_caught_when_shapes_alternate(oracle):
    """Calls of two shapes alternate on one context: 32 blocks of 1 KiB (S = 16, a period of two calls) and a single short block.  The
    rotation is counted per shape, so the victim — block 1, sampled only by odd rotations — is caught at the second call of its shape
    (with one count for the context, the 32-block calls would only ever take even rotations)."""
    bs = 1024
    a_data, b_data = markov_text(32 * bs, seed=51), lcg_text(500, seed=52)
    dev, orc = pair(oracle, "order0")
    want_a = oracle.encode_blocks(orc(), a_data, bs, nthreads=8)
    want_b = oracle.encode_blocks(orc(), b_data, bs, nthreads=8)
    c = _faulty_ctx(None, 1)
    try:
        c.set_path("twophase")

        def a_then_b():
            r = _encode(c, dev(), a_data, bs)
            b_out, _, b_faults = _encode(c, dev(), b_data, bs)
            assert b_faults == 0 and b_out.tobytes() == want_b[0].tobytes()   # (one block: the victim is not in it)
            return r
        caught = _caught_at([a_then_b] * 2, 1, want_a)
        assert caught == first_sampled(32, False, bs, 1, 1) == 1
    finally:
        c.close()


def test_a_fault_is_caught_in_any_piece_of_a_chunked_call(oracle):
    """w3_encode_blocks in pieces (W3_OPT_HOST_CHUNK_BLOCKS = 32 over 32 blocks and a short one: a piece of 32 blocks, S = 16, a period
    of two calls, and a piece of one block).  Every piece takes the host call's number for the rotation, so block 1 of the first piece
    — sampled only by odd rotations — is caught at the second call (with one number per piece, the first piece would only ever take
    even rotations)."""
    bs = 1024
    data = markov_text(32 * bs + 500, seed=53)
    dev, orc = pair(oracle, "order0")
    want = oracle.encode_blocks(orc(), data, bs, nthreads=8)
    c = _faulty_ctx(None, 1)
    try:
        c.set_path("twophase")
        c.set_host_chunk_blocks(32)

        def call():
            r = _encode(c, dev(), data, bs)
            assert c.timing()["n_parts"] == 2
            return r
        caught = _caught_at([call] * 2, 1, want)
        assert caught == first_sampled(32, False, bs, 1, 1) == 1
        out, lens = c.encode_blocks(dev(), data, bs)
        assert c.timing()["n_lds_faults"] == 0 and out.tobytes() == want[0].tobytes()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# C.3 recovery at every entry point (fault in every block, all three kernels)
# ---------------------------------------------------------------------------------------------------------------------------------
def _d_out(bufs):
    d_out, d_lens, d_total = bufs
    return d_out[: int(d_total.item())].cpu().numpy().tobytes(), d_lens


@pytest.mark.parametrize("name", ["best012", "o012_apm"])
def test_recovery_submit_wait_two_jobs_in_flight(oracle, name):
    import torch
    bs = 4096
    datas = [markov_text(300 * 1024 + 333, seed=31) + lcg_text(100 * 1024, seed=6), lcg_text(200 * 1024 + 7, seed=9) + markov_text(150 * 1024, seed=32)]
    dev, orc = _o012_apm(oracle) if name == "o012_apm" else pair(oracle, name)
    want = [oracle.encode_blocks(orc(), d, bs, nthreads=8) for d in datas]
    d_ins = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in datas]
    bufs = _device_bufs(max(len(d) for d in datas), bs, 2)
    torch.cuda.synchronize()
    c = _faulty_ctx()
    try:
        c.set_tune(4096)   # the ordered pair (two jobs in flight, as bench.py runs them)
        jobs = [c.encode_submit(dev(), d_ins[k], bs, *bufs[k]) for k in range(2)]
        faults = []
        for k in range(2):
            c.encode_wait(jobs[k])
            faults.append(c.timing()["n_lds_faults"])
            out, d_lens = _d_out(bufs[k])
            assert d_lens[:len(want[k][1])].cpu().numpy().astype(np.uint32).tolist() == want[k][1].tolist(), k
            assert out == want[k][0].tobytes(), k
        assert faults[0] > 0, faults
        for rnd in range(2):   # every job slot now runs the ballot path
            jobs = [c.encode_submit(dev(), d_ins[k], bs, *bufs[k]) for k in range(2)]
            for k in range(2):
                c.encode_wait(jobs[k])
                assert c.timing()["n_lds_faults"] == 0, (rnd, k)
                assert _d_out(bufs[k])[0] == want[k][0].tobytes(), (rnd, k)
    finally:
        c.close()


def test_recovery_submit_wait_four_free_running_jobs(oracle):
    import torch
    bs = 2048
    datas = [markov_text(200 * 1024 + 333, seed=41) + bytes(30 * 1024), lcg_text(150 * 1024 + 7, seed=19) + markov_text(90 * 1024, seed=42),
             markov_text(64 * 1024 + 1, seed=43), lcg_text(100 * 1024 + 99, seed=44)]
    names = ["best012", "o012_apm", "order1", "main_default"]
    mk = lambda nm: _o012_apm(oracle) if nm == "o012_apm" else pair(oracle, nm)
    want = [oracle.encode_blocks(mk(names[k])[1](), datas[k], bs, nthreads=8) for k in range(4)]
    d_ins = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in datas]
    bufs = _device_bufs(max(len(d) for d in datas), bs, 4)
    torch.cuda.synchronize()
    c = _faulty_ctx()
    try:
        assert c.max_in_flight(len(datas[0]), bs) == 4
        for rnd in range(2):
            jobs = [c.encode_submit(mk(names[k])[0](), d_ins[k], bs, *bufs[k]) for k in range(4)]
            faults = []
            for k in (0, 2, 3, 1):   # out of order
                c.encode_wait(jobs[k])
                faults.append(c.timing()["n_lds_faults"])
                out, d_lens = _d_out(bufs[k])
                assert d_lens[:len(want[k][1])].cpu().numpy().astype(np.uint32).tolist() == want[k][1].tolist(), (rnd, k)
                assert out == want[k][0].tobytes(), (rnd, names[k])
            if rnd == 0:
                assert faults[0] > 0, faults
            else:
                assert faults == [0, 0, 0, 0], faults   # every job slot on the ballot path
    finally:
        c.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_recovery_host_submit_wait(oracle, pinned):
    import torch
    bs = 2048
    datas = [markov_text(200 * 1024 + 333, seed=81) + bytes(30 * 1024), lcg_text(150 * 1024 + 7, seed=29) + markov_text(90 * 1024, seed=82)]
    dev, orc = pair(oracle, "best012")
    want = [oracle.encode_blocks(orc(), d, bs, nthreads=8) for d in datas]
    cap = 2 * max(len(d) for d in datas) + 8192
    if pinned:
        ins = []
        for d in datas:
            t = torch.empty(len(d), dtype=torch.uint8).pin_memory()
            t.numpy()[:] = np.frombuffer(d, dtype=np.uint8)
            ins.append(t)
        outs = [(torch.empty(cap, dtype=torch.uint8).pin_memory(), torch.empty(256, dtype=torch.int32).pin_memory()) for _ in range(3)]
        view = lambda o, m: o.numpy()[:m]
    else:
        ins = [np.frombuffer(d, dtype=np.uint8).copy() for d in datas]
        outs = [(np.zeros(cap, dtype=np.uint8), np.zeros(256, dtype=np.uint32)) for _ in range(3)]
        view = lambda o, m: o[:m]
    c = _faulty_ctx()
    try:
        for rnd in range(2):
            seq = [0, 1, 0]
            jobs = [c.encode_host_submit(dev(), ins[k], bs, *outs[i]) for i, k in enumerate(seq)]
            faults = []
            for i, k in enumerate(seq):
                total = c.encode_host_wait(jobs[i])
                faults.append(c.timing()["n_lds_faults"])
                o, ln = outs[i]
                assert total == len(want[k][0]), (rnd, i)
                assert view(ln, len(want[k][1])).astype(np.uint32).tolist() == want[k][1].tolist(), (rnd, i)
                assert view(o, total).tobytes() == want[k][0].tobytes(), (rnd, i)
            assert (faults[0] > 0) if rnd == 0 else faults == [0, 0, 0], (rnd, faults)
    finally:
        c.close()


def test_recovery_encode_blocks_in_pieces(oracle):
    """w3_encode_blocks in pieces of 7 blocks over 42 (the last one short): pieces in flight, each of them faulting."""
    bs = 4096
    data = markov_text(41 * bs + 1234, seed=91)
    dev, orc = pair(oracle, "best012")
    want, wlens = oracle.encode_blocks(orc(), data, bs, nthreads=8)
    c = _faulty_ctx()
    try:
        c.set_host_chunk_blocks(7)
        out, lens = c.encode_blocks(dev(), data, bs)
        assert c.timing()["n_parts"] == 6 and c.timing()["n_lds_faults"] > 0
        assert lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes()
        out, lens = c.encode_blocks(dev(), data, bs)
        assert c.timing()["n_lds_faults"] == 0 and lens.tolist() == wlens.tolist() and out.tobytes() == want.tobytes()
    finally:
        c.close()


def test_recovery_sharded_encode(oracle):
    """w3_encode_blocks_sharded over three contexts on the one device, every one of them faulting."""
    cs = [_faulty_ctx() for _ in range(3)]
    try:
        n, bs = 150000, 4096
        data = np.frombuffer(markov_text(n, seed=27), dtype=np.uint8)
        nb = (n + bs - 1) // bs
        dev, orc = pair(oracle, "best012")
        want, wlens = oracle.encode_blocks(orc(), bytes(data), bs, nthreads=8)
        spec = dev().spec()
        hs = (C.c_void_p * 3)(*[c.h for c in cs])
        for rnd in range(2):
            out = np.zeros(2 * n + 64 * nb + 64, dtype=np.uint8)
            lens = np.zeros(nb, dtype=np.uint32)
            olen = C.c_size_t()
            rc = cs[0].lib.w3_encode_blocks_sharded(hs, 3, C.byref(spec), data.ctypes.data_as(C.c_void_p), n, bs, out.ctypes.data_as(C.c_void_p),
                                                    len(out), C.byref(olen), lens.ctypes.data_as(C.c_void_p))
            assert rc == 0, cs[0].lib.w3_last_error(cs[0].h)
            assert lens.tolist() == wlens.tolist() and out[:olen.value].tobytes() == want.tobytes(), rnd
            faults = [c.timing()["n_lds_faults"] for c in cs]
            assert (sum(faults) > 0) if rnd == 0 else faults == [0, 0, 0], (rnd, faults)
    finally:
        for c in cs:
            c.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# C.4 the ballot path a context lands on after a fault
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ballot_ctx():
    c = w3.Context(0)
    c.set_variant("no_lds_atomics")
    yield c
    c.close()


@pytest.mark.parametrize("name", TWOPHASE)
def test_ballot_path_models(ballot_ctx, oracle, name):
    data = markov_text(150000, seed=22) + bytes(66000) + lcg_text(9000, seed=5)
    check_blocks(ballot_ctx, oracle, name, data, 65536, "twophase")
    dev, orc = pair(oracle, name)
    bs = 16384
    p = ballot_ctx.predict_blocks(dev(), data[:40000], bs)
    assert np.array_equal(p, np.concatenate([oracle.predict_all(orc(), data[o:min(o + bs, 40000)]) for o in range(0, 40000, bs)])), name


def test_ballot_path_block_sizes(ballot_ctx, oracle):
    """The block sizes of the x5 coder loop (ragged and tiny blocks), and blocks above 64 KiB (4-bit partition passes over more than
    2^16 positions): 1 MiB and 4 MiB + 12,345 bytes."""
    data = markov_text(60000, seed=31) + bytes(5000) + np.random.default_rng(2).integers(0, 256, 20000, dtype=np.uint8).tobytes()
    tail = markov_text(3 * 8192 + 5, seed=77) + b"ab"
    for name in ("order0", "best012", "best_ac_wide"):
        for d_, bs_ in ((data, 8192), (tail, 8192), (tail[:8195], 4099), (tail[:700], 7), (tail[:64 * 13 + 3], 13)):
            check_blocks(ballot_ctx, oracle, name, d_, bs_, "twophase")
    big = markov_text(2 * (1 << 20) + 777, seed=33)
    check_blocks(ballot_ctx, oracle, "best012", big, 1 << 20, "twophase")
    big = markov_text((4 << 20) + 12345, seed=34)
    check_blocks(ballot_ctx, oracle, "best012", big, 4 << 20, "twophase")


def test_ballot_path_counter_saturation(ballot_ctx, oracle):
    from tests.test_gpu_parity import saturation_cases
    for cname, (data, bs) in saturation_cases().items():
        for name in ("order0", "best012", "main_default"):
            check_blocks(ballot_ctx, oracle, name, data, bs, "twophase")


@pytest.mark.parametrize("name", ["o012_apm", "slot1", "slot_mix", "apm_chain4"])
def test_ballot_path_cm_models(ballot_ctx, oracle, name):
    """The APM and slot-state models, both decoders (tests/test_gpu_cm.py::check); under no_lds_atomics the slot leaves run on k_slot
    instead of the sorted replay."""
    from tests.test_gpu_cm import check
    data = markov_text(100000, seed=12) + bytes(3000) + lcg_text(20000, seed=13)
    check(ballot_ctx, oracle, name, data, 16384, variant=("no_lds_atomics",))
