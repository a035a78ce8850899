"""AC over Huffman on the device (w3_aoh_*; bin/ac-over-huffman/main.rs:69-89) against the CPU truth of tests/aoh_ref.py, byte for byte:
streams, length tables, ACStats bit counts, decode, the sweep, refusals, the CLI's version-2 container.  Every case runs on each
path that is built: the fused lane-per-block kernel (W3_PATH_GENERIC) and, when the library has one, the two-phase form.  The
host-buffer calls go through in runs of whole blocks, one device call each; W3_OPT_HOST_CHUNK_BLOCKS sets the run length."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L
from tests import aoh_ref
from tests.synth import markov_text, mixed_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twophase_built():
    """One module-level condition: W3_PATH_TWOPHASE answers W3_E_UNSUPPORTED for this family when the two-phase form is left out."""
    import torch
    if not torch.cuda.is_available():
        return False
    ctx = w3.Context(0)
    try:
        ctx.set_path("twophase")
        try:
            ctx.aoh_encode_stats(w3.HuffCode.new(b"abracadabra", 8), 8, b"abracadabra", 64)
        except w3.W3Error as e:
            if e.code == L.W3_E_UNSUPPORTED:
                return False
            raise
        return True
    finally:
        ctx.close()


PATHS = ["generic"] + (["twophase"] if _twophase_built() else [])


@pytest.fixture(scope="module")
def ctx():
    c = w3.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("aoh_ref")


@pytest.fixture(scope="module")
def text():
    return markov_text(1000003, seed=3)      # 1,000,000 B + a ragged tail


def _code(codes, lens):
    return w3.HuffCode.from_tables(codes, lens)


def _all_paths(ctx, code, cb, data, bs):
    """encode + stats + decode on every built path; the paths' outputs equal each other.  -> (streams bytes, lens, bits)"""
    res = []
    for path in PATHS:
        ctx.set_path(path)
        try:
            out, lens = ctx.aoh_encode_blocks(code, cb, data, bs)
            bits = ctx.aoh_encode_stats(code, cb, data, bs)
            back = ctx.aoh_decode_blocks(code, cb, out, lens, bs, len(data))
        finally:
            ctx.set_path("auto")
        assert back.tobytes() == bytes(data), path
        res.append((out.tobytes(), lens.tolist(), bits.tolist()))
    for r in res[1:]:
        assert r == res[0]
    return res[0]


def _check_against_truth(ctx, oracle, build_dir, codes, lens, cb, data, bs):
    code = _code(codes, lens)
    want, wlens = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, cb, data, bs)
    wbits = aoh_ref.stats_bits(oracle, build_dir, codes, lens, cb, data, bs)
    got, glens, gbits = _all_paths(ctx, code, cb, data, bs)
    assert glens == wlens.tolist()
    assert got == want
    assert gbits == wbits.tolist()
    # the device decodes the CPU truth's streams too
    for path in PATHS:
        ctx.set_path(path)
        try:
            assert ctx.aoh_decode_blocks(code, cb, np.frombuffer(want, dtype=np.uint8), wlens, bs, len(data)).tobytes() == bytes(data)
        finally:
            ctx.set_path("auto")


@pytest.mark.parametrize("bs", [4096, 65536, 262144])
@pytest.mark.parametrize("hsize", [6, 9, 13])
def test_parity_text(ctx, oracle, build_dir, text, bs, hsize):
    """ctx_bits 1 .. 31: direct table, exact map, and the start where fewer than ctx_bits bits have been seen"""
    codes, lens = aoh_ref.code_table(oracle, text, hsize)
    for cb in (1, 8, 16, 19, 24, 31):
        _check_against_truth(ctx, oracle, build_dir, codes, lens, cb, text, bs)


def test_parity_mixed_bytes(ctx, oracle, build_dir):
    data = mixed_bytes(512 * 1024, seed=7)
    codes, lens = aoh_ref.code_table(oracle, data, 9)
    _check_against_truth(ctx, oracle, build_dir, codes, lens, 16, data, 65536)


def test_halving(ctx, oracle, build_dir):
    """300,000 equal bytes plus one other symbol at the end: the two-symbol table, one context hit more than 65,535 times"""
    data = b"a" * 300000 + b"b"
    codes, lens = aoh_ref.code_table(oracle, data, 12)
    assert (codes[97], lens[97], codes[98], lens[98]) == (0, 1, 1, 1)
    for cb in (1, 8):
        _check_against_truth(ctx, oracle, build_dir, codes, lens, cb, data, 1 << 19)


@pytest.mark.parametrize("cb", [8, 16, 22])
def test_identity_table_equals_the_existing_ordern_path(ctx, cb):
    """code[s] = s, len 8 (canonical of 256 equal lengths): the new path's streams are encode_blocks(OrderN(ctx_bits, 0))'s"""
    data = markov_text(300000 + 17, seed=9) + mixed_bytes(100000, seed=10)
    codes, lens = aoh_ref.identity_table()
    want, wlens = ctx.encode_blocks(w3.OrderN(cb, 0), data, 65536)
    wbits = ctx.encode_stats(w3.OrderN(cb, 0), data, 65536)
    got, glens, gbits = _all_paths(ctx, _code(codes, lens), cb, data, 65536)
    assert glens == wlens.tolist() and got == want.tobytes() and gbits == wbits.tolist()


@pytest.mark.parametrize("n", [0, 1, 4096, 4097])
def test_edge_sizes(ctx, oracle, build_dir, text, n):
    """empty input, n = 1, n = block_size, n = block_size + 1"""
    codes, lens = aoh_ref.code_table(oracle, text, 9)
    data = text[:n]
    if n == 0:
        for path in PATHS:
            ctx.set_path(path)
            try:
                out, bl = ctx.aoh_encode_blocks(_code(codes, lens), 16, data, 4096)
                assert len(out) == 0 and len(bl) == 0
                assert len(ctx.aoh_encode_stats(_code(codes, lens), 16, data, 4096)) == 0
                assert len(ctx.aoh_decode_blocks(_code(codes, lens), 16, out, bl, 4096, 0)) == 0
            finally:
                ctx.set_path("auto")
        return
    _check_against_truth(ctx, oracle, build_dir, codes, lens, 16, data, 4096)


def test_device_resident_entry_points(ctx, oracle, build_dir, text):
    import torch
    data = text[:300000 + 5]
    bs = 65536
    codes, lens = aoh_ref.code_table(oracle, data, 9)
    code = _code(codes, lens)
    want, wlens = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, 19, data, bs)
    wbits = aoh_ref.stats_bits(oracle, build_dir, codes, lens, 19, data, bs)
    nb = len(wlens)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    for path in PATHS:
        ctx.set_path(path)
        try:
            d_out = torch.zeros(len(data) * 2 + 1024, dtype=torch.uint8, device="cuda")
            d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
            d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
            ctx.set_timing(True)
            ctx.aoh_encode_blocks_device(code, 19, d_in, bs, d_out, d_lens, d_total)
            tm = ctx.timing()
            ctx.set_timing(False)
            assert tm["total_ms"] > 0 and tm["n_parts"] == 1
            total = int(d_total.item())
            assert total == len(want) and d_lens.cpu().numpy().astype(np.uint32).tolist() == wlens.tolist()
            assert d_out[:total].cpu().numpy().tobytes() == want
            d_bits = torch.zeros(nb, dtype=torch.int32, device="cuda")
            ctx.aoh_encode_stats_device(code, 19, d_in, bs, d_bits)
            assert d_bits.cpu().numpy().astype(np.uint32).tolist() == wbits.tolist()
            d_back = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
            ctx.aoh_decode_blocks_device(code, 19, d_out[:total], d_lens, bs, len(data), d_back)
            assert d_back.cpu().numpy().tobytes() == data
            # out_cap too small: W3_E_NOSPACE, d_total = the need, nothing written past out_cap
            cap = total - 1000
            d_small = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            d_total.zero_()
            rc = ctx.lib.w3_aoh_encode_blocks_device(ctx.h, C.byref(code.table), 19, C.c_void_p(d_in.data_ptr()), len(data), bs, C.c_void_p(d_small.data_ptr()),
                                                     cap, C.c_void_p(d_lens.data_ptr()), C.c_void_p(d_total.data_ptr()), None)
            assert rc == L.W3_E_NOSPACE and int(d_total.item()) == total
            assert bool((d_small[cap:] == 0xA5).all())
        finally:
            ctx.set_timing(False)
            ctx.set_path("auto")


def test_refusals(ctx, oracle, build_dir, text):
    import torch
    data = text[:200000]
    bs = 65536
    codes, lens = aoh_ref.code_table(oracle, data, 9)
    code = _code(codes, lens)
    a = np.frombuffer(data, dtype=np.uint8)
    nb = (len(a) + bs - 1) // bs
    for path in PATHS:
        ctx.set_path(path)
        try:
            # a byte whose len is 0: encode refuses, the counting sink mirrors the reference (the byte contributes no bits)
            bad = data[:100000] + b"\x00" + data[100000:]
            assert lens[0] == 0
            with pytest.raises(w3.W3Error) as e:
                ctx.aoh_encode_blocks(code, 16, bad, bs)
            assert e.value.code == L.W3_E_INVALID
            assert ctx.aoh_encode_stats(code, 16, bad, bs).tolist() == aoh_ref.stats_bits(oracle, build_dir, codes, lens, 16, bad, bs).tolist()
            # out_cap too small (host buffers): W3_E_NOSPACE, *out_len = the need, nothing written past out_cap
            out, bl = ctx.aoh_encode_blocks(code, 16, data, bs)
            cap = len(out) - 500
            small = np.full(len(out) + 64, 0xA5, dtype=np.uint8)
            gl = np.zeros(nb, dtype=np.uint32)
            olen = C.c_size_t()
            rc = ctx.lib.w3_aoh_encode_blocks(ctx.h, C.byref(code.table), 16, a.ctypes.data_as(C.c_void_p), len(a), bs, small.ctypes.data_as(C.c_void_p), cap,
                                              C.byref(olen), gl.ctypes.data_as(C.c_void_p))
            assert rc == L.W3_E_NOSPACE and olen.value == len(out) and gl.tolist() == bl.tolist()
            assert (small[cap:] == 0xA5).all()
            # a length table that claims more than in_len
            with pytest.raises(w3.W3Error) as e:
                ctx.aoh_decode_blocks(code, 16, out[:len(out) - 10], bl, bs, len(data))
            assert e.value.code == L.W3_E_FORMAT
            d_comp = torch.from_numpy(out.copy()).cuda()
            d_lens = torch.from_numpy(bl.astype(np.int32)).cuda()
            d_back = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
            with pytest.raises(w3.W3Error) as e:
                ctx.aoh_decode_blocks_device(code, 16, d_comp[:len(out) - 10], d_lens, bs, len(data), d_back)
            assert e.value.code == L.W3_E_FORMAT
            # invalid arguments: ctx_bits, the table, nblocks
            for cb in (0, 32):
                with pytest.raises(w3.W3Error) as e:
                    ctx.aoh_encode_stats(code, cb, data, bs)
                assert e.value.code == L.W3_E_INVALID
            broken = list(codes)
            broken[max(range(256), key=lambda s: lens[s])] ^= 1
            with pytest.raises(w3.W3Error) as e:
                ctx.aoh_encode_blocks(_code(broken, lens), 16, data, bs)
            assert e.value.code == L.W3_E_INVALID
            with pytest.raises(w3.W3Error) as e:
                ctx.aoh_decode_blocks(code, 16, out, bl[:-1], bs, len(data))
            assert e.value.code == L.W3_E_INVALID
        finally:
            ctx.set_path("auto")
    # a call while w3_encode_submit has a job in flight
    d_in = torch.from_numpy(a.copy()).cuda()
    d_out = torch.zeros(2 * len(a) + 1024, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    job = ctx.encode_submit(w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3)), d_in, bs, d_out, d_lens, d_total)
    try:
        for call in (lambda: ctx.aoh_encode_blocks(code, 16, data, bs), lambda: ctx.aoh_encode_stats(code, 16, data, bs),
                     lambda: ctx.aoh_decode_blocks(code, 16, out, bl, bs, len(data)),
                     lambda: ctx.sweep_ac_over_huffman(data, bs, [code], [(0, 16)])):
            with pytest.raises(w3.W3Error) as e:
                call()
            assert e.value.code == L.W3_E_INVALID
    finally:
        ctx.encode_wait(job)
    assert ctx.aoh_decode_blocks(code, 16, out, bl, bs, len(data)).tobytes() == data


def test_single_symbol_input_through_the_container_writer(ctx):
    """The reference's table for one distinct symbol is all zero (the file codes zero bits): encode refuses it, stats report 0 bits,
    and the container writer's replacement (len 1, code 0) round-trips."""
    data = b"q" * 70001
    zero = w3.HuffCode.new(data, 12)
    assert not any(zero.lens)
    assert ctx.aoh_encode_stats(zero, 16, data, 65536).tolist() == [0, 0]
    with pytest.raises(w3.W3Error) as e:
        ctx.aoh_encode_blocks(zero, 16, data, 65536)
    assert e.value.code == L.W3_E_INVALID
    code, out, lens = ctx.aoh_compress(data, 12, 16, 65536)
    assert code.lens[ord("q")] == 1 and sum(code.lens) == 1
    assert ctx.aoh_decode_blocks(code, 16, out, lens, 65536, len(data)).tobytes() == data


def test_sweep_in_one_call(ctx, oracle, build_dir):
    """huffman_size 7..15 x ctx_bits 8..30 on 256 KiB in 16 KiB blocks, ONE call: every row equals w3_aoh_encode_stats of its configuration
    and the CPU truth's bits; sweep.py prints the minimum of the table under the reference's tie rule"""
    import torch
    from weath3rb0i_amd import sweep
    data = markov_text(256 * 1024, seed=21)
    bs = 16384
    hsizes, cbs = list(range(7, 16)), list(range(8, 31))
    tabs = [aoh_ref.code_table(oracle, data, h) for h in hsizes]
    codes = [_code(c, l) for c, l in tabs]
    configs = [(k, b) for k in range(len(codes)) for b in cbs]
    rows = ctx.sweep_ac_over_huffman(data, bs, codes, configs)
    assert rows.shape == (len(configs), 16)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    assert (ctx.sweep_ac_over_huffman_device(d_in, bs, codes, configs) == rows).all()
    for (k, b), row in zip(configs, rows):
        assert row.tolist() == ctx.aoh_encode_stats(codes[k], b, data, bs).tolist(), (hsizes[k], b)
        assert row.tolist() == aoh_ref.stats_bits(oracle, build_dir, tabs[k][0], tabs[k][1], b, data, bs).tolist(), (hsizes[k], b)
    lines = []
    best, params, table = sweep.sweep_ac_over_huffman(ctx, data, bs, out=lines.append)
    csize = {(hsizes[k], b): int(row.astype(np.uint64).sum()) // 8 for (k, b), row in zip(configs, rows)}
    assert table == csize
    lo = min(csize.values())
    last = [hb for hb in ((h, b) for h in hsizes for b in cbs) if csize[hb] == lo][-1]     # a later configuration replaces an equal one
    assert (best, params) == (lo, last)
    assert lines[-1] == "-> gloabl best: %d for [hsize: %d, ctx: %d, align: 0]" % (lo, last[0], last[1])
    assert sum(ln.startswith("[ac-over-huff] [hsize:") for ln in lines) == len(configs) and sum(ln.startswith("-> best:") for ln in lines) == len(hsizes)


def test_cli_version_2_container(ctx, oracle, build_dir, tmp_path):
    cli = os.path.join(ROOT, "tools", "w3")
    src = os.path.join(ROOT, "tools", "w3cli.cpp")
    if not os.path.exists(cli) or os.path.getmtime(cli) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", cli, src, "-L" + os.path.join(ROOT, "weath3rb0i_amd"), "-lw3hip",
                               "-Wl,-rpath,$ORIGIN/../weath3rb0i_amd", "-Wl,-rpath,/opt/rocm/lib"])

    def run(*args, **env):
        e = dict(os.environ)
        e.update(env)
        return subprocess.run([cli, *args], cwd=tmp_path, env=e, capture_output=True, text=True, timeout=300)

    data = markov_text(200000, seed=31) + mixed_bytes(70000, seed=32)
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)
    r = run("t", str(f), W3_MODEL="aoh:9,16")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "corpus.orig").read_bytes() == data
    blob = (tmp_path / "corpus.bin").read_bytes()
    assert blob[:5] == b"w3bk\x02"
    orig, bs, nb = int.from_bytes(blob[5:13], "big"), int.from_bytes(blob[13:17], "big"), int.from_bytes(blob[17:21], "big")
    assert (orig, bs, nb) == (len(data), 65536, 5) and blob[21] == 16
    codes = [int.from_bytes(blob[22 + 2 * s:24 + 2 * s], "big") for s in range(256)]
    lens = list(blob[22 + 512:22 + 768])
    assert (codes, lens) == aoh_ref.code_table(oracle, data, 9)
    hdr = 21 + 769
    bl = [int.from_bytes(blob[hdr + 4 * b:hdr + 4 * b + 4], "big") for b in range(nb)]
    want, wlens = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, 16, data, 65536)
    assert bl == wlens.tolist() and blob[hdr + 4 * nb:] == want
    # random access is not built for these streams: a message and a non-zero exit
    r = run("r", str(tmp_path / "corpus.bin"), "10", "100")
    assert r.returncode != 0 and "random access is not implemented" in r.stderr
    # the default model still writes and reads version 1
    (tmp_path / "corpus.orig").unlink()
    r = run("t", str(f))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "corpus.bin").read_bytes()[:5] == b"w3bk\x01" and (tmp_path / "corpus.orig").read_bytes() == data
    # a one-symbol file and an empty file through the writer
    for name, content in (("one.txt", b"z" * 70000), ("empty.txt", b"")):
        g = tmp_path / name
        g.write_bytes(content)
        r = run("t", str(g), W3_MODEL="aoh")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / (name[:-4] + ".orig")).read_bytes() == content


def test_host_calls_in_runs(ctx, oracle, build_dir, text):
    """10 blocks of 1,024 bytes and a 77-byte tail under W3_OPT_HOST_CHUNK_BLOCKS = 3 (four runs, the last of two blocks, one ragged), 1 (a
    run per block) and 64 (one run), and without the option: encode, the counting sink and decode equal the CPU truth whatever the runs."""
    bs, cb = 1024, 12
    data = text[:10 * bs + 77]
    codes, lens = aoh_ref.code_table(oracle, text, 12)
    code = _code(codes, lens)
    want, wlens = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, cb, data, bs)
    wbits = aoh_ref.stats_bits(oracle, build_dir, codes, lens, cb, data, bs)
    assert len(wlens) == 11
    try:
        for runs_of in (3, 1, 64, 0):
            ctx.set_host_chunk_blocks(runs_of)
            out, glens = ctx.aoh_encode_blocks(code, cb, data, bs)
            assert ctx.timing()["n_parts"] == ((11 + runs_of - 1) // runs_of if runs_of else 1), runs_of
            assert glens.tolist() == wlens.tolist() and out.tobytes() == want, runs_of
            assert ctx.aoh_encode_stats(code, cb, data, bs).tolist() == wbits.tolist(), runs_of
            assert ctx.aoh_decode_blocks(code, cb, np.frombuffer(want, dtype=np.uint8), wlens, bs, len(data)).tobytes() == bytes(data), runs_of
    finally:
        ctx.set_host_chunk_blocks(0)
