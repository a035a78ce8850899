"""`w3 c` under W3_MODEL=aoh takes its code table from the device's histogram (w3_histogram + w3_huff_code_from_counts): the container
equals the one assembled from HuffCode.new on the host, byte for byte, and `w3 d` restores the file."""
import os
import subprocess

import pytest

import weath3rb0i_amd as w3
from tests.synth import markov_text, mixed_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "w3")
BS = 65536


@pytest.fixture(scope="module")
def cli():
    src = os.path.join(ROOT, "tools", "w3cli.cpp")
    if not os.path.exists(CLI) or os.path.getmtime(CLI) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", CLI, src, "-L" + os.path.join(ROOT, "weath3rb0i_amd"), "-lw3hip",
                               "-Wl,-rpath,$ORIGIN/../weath3rb0i_amd", "-Wl,-rpath,/opt/rocm/lib"])
    return CLI


def run(cli, cwd, *args, **env):
    e = dict(os.environ)
    e.pop("W3_CHECK", None)
    e.update(env)
    return subprocess.run([cli, *args], cwd=cwd, env=e, capture_output=True, text=True, timeout=300)


def container(data, code, ctx_bits, streams, lens):
    """version 2 of `w3bk` (tools/w3cli.cpp write_block_container)"""
    out = b"w3bk" + bytes([2]) + len(data).to_bytes(8, "big") + BS.to_bytes(4, "big") + len(lens).to_bytes(4, "big") + bytes([ctx_bits])
    out += b"".join(int(c).to_bytes(2, "big") for c in code.codes) + bytes(code.lens)
    return out + b"".join(int(x).to_bytes(4, "big") for x in lens) + streams


@pytest.mark.parametrize("hsize,ctx_bits,kind", [(12, 16, "text"), (9, 20, "mixed"), (13, 24, "one")])
def test_aoh_container_from_the_device_histogram(cli, tmp_path, hsize, ctx_bits, kind):
    data = {"text": markov_text(200001, seed=41), "mixed": markov_text(70000, seed=42) + mixed_bytes(100000, seed=43), "one": b"z" * 70001}[kind]
    (tmp_path / "in").mkdir()
    f = tmp_path / "in" / "corpus.txt"
    f.write_bytes(data)
    model = "aoh:%d,%d" % (hsize, ctx_bits)
    r = run(cli, tmp_path, "c", str(f), W3_MODEL=model)
    assert r.returncode == 0, r.stderr
    blob = (tmp_path / "corpus.bin").read_bytes()
    code = w3.HuffCode.new(data, hsize)   # the histogram loop on the host
    if not any(code.lens):
        code = code.with_single_symbol(data[0])
    ctx = w3.Context(0)
    try:
        streams, lens = ctx.aoh_encode_blocks(code, ctx_bits, data, BS)
    finally:
        ctx.close()
    assert blob == container(data, code, ctx_bits, streams.tobytes(), lens.tolist())
    r = run(cli, tmp_path, "d", str(tmp_path / "corpus.bin"), W3_MODEL=model)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "corpus.orig").read_bytes() == data
