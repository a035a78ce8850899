"""The CLI's checked containers (tools/w3cli.cpp, W3_CHECK=1: versions 3 and 4 of `w3bk`) on the GPU: the CRC table and the header CRC
against zlib, the streams against the unchecked file's, and what `w3 d` and `w3 r` do with a damaged file."""
import os
import subprocess
import zlib

import pytest

from tests.synth import markov_text, mixed_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "w3")
BS = 65536


@pytest.fixture(scope="module")
def cli():
    src = os.path.join(ROOT, "tools", "w3cli.cpp")
    hdr = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_crc.h")
    if not os.path.exists(CLI) or os.path.getmtime(CLI) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", CLI, src, "-L" + os.path.join(ROOT, "weath3rb0i_amd"), "-lw3hip",
                               "-Wl,-rpath,$ORIGIN/../weath3rb0i_amd", "-Wl,-rpath,/opt/rocm/lib"])
    return CLI


def run(cli, cwd, *args, **env):
    e = dict(os.environ)
    e.pop("W3_CHECK", None)
    e.update(env)
    return subprocess.run([cli, *args], cwd=cwd, env=e, capture_output=True, text=True, timeout=300)


def parse(blob):
    """-> dict of a `w3bk` file's parts (any version)"""
    assert blob[:4] == b"w3bk"
    v = blob[4]
    orig, bs, nb = int.from_bytes(blob[5:13], "big"), int.from_bytes(blob[13:17], "big"), int.from_bytes(blob[17:21], "big")
    hdr = 21 + (769 if v in (2, 4) else 0)
    lens = [int.from_bytes(blob[hdr + 4 * b:hdr + 4 * b + 4], "big") for b in range(nb)]
    p = hdr + 4 * nb
    out = {"version": v, "orig": orig, "bs": bs, "nb": nb, "model": blob[21:hdr], "lens": lens, "lens_at": hdr}
    if v >= 3:
        out["crc"] = [int.from_bytes(blob[p + 4 * b:p + 4 * b + 4], "big") for b in range(nb)]
        out["crc_at"] = p
        p += 4 * nb
        out["header_crc"], out["header_bytes"] = int.from_bytes(blob[p:p + 4], "big"), blob[:p]
        p += 4
    out["streams_at"], out["streams"] = p, blob[p:]
    return out


def flipped(blob, at):
    b = bytearray(blob)
    b[at] ^= 0x40
    return bytes(b)


@pytest.mark.parametrize("model,version", [("default", 3), ("aoh:9,16", 4)])
def test_checked_container_round_trip_and_damage(cli, tmp_path, model, version):
    data = markov_text(3 * BS, seed=81) + mixed_bytes(BS + 4321, seed=82)
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)
    assert run(cli, tmp_path, "c", str(f), W3_MODEL=model).returncode == 0
    plain = parse((tmp_path / "corpus.bin").read_bytes())
    assert plain["version"] == version - 2                                       # without W3_CHECK: versions 1 and 2 as before
    r = run(cli, tmp_path, "t", str(f), W3_MODEL=model, W3_CHECK="1")
    assert r.returncode == 0, r.stderr
    blob = (tmp_path / "corpus.bin").read_bytes()
    assert blob[:5] == b"w3bk" + bytes([version])
    c = parse(blob)
    assert (tmp_path / "corpus.orig").read_bytes() == data
    assert c["crc"] == [zlib.crc32(data[o:o + BS]) for o in range(0, len(data), BS)]
    assert c["header_crc"] == zlib.crc32(c["header_bytes"])
    assert (c["orig"], c["bs"], c["nb"], c["model"], c["lens"], c["streams"]) == (plain["orig"], plain["bs"], plain["nb"], plain["model"], plain["lens"], plain["streams"])
    # a byte flipped in block 2's stream: `w3 d` names the block and writes nothing
    (tmp_path / "corpus.orig").unlink()
    at = c["streams_at"] + sum(c["lens"][:2]) + c["lens"][2] // 2
    (tmp_path / "corpus.bin").write_bytes(flipped(blob, at))
    r = run(cli, tmp_path, "d", str(tmp_path / "corpus.bin"), W3_MODEL=model)
    assert r.returncode != 0 and "block 2 " in r.stderr and "CRC-32" in r.stderr, r.stderr
    assert not (tmp_path / "corpus.orig").exists()
    # a byte flipped in the length table or in the CRC table: the header message, before anything is decoded
    for at in (c["lens_at"] + 5, c["crc_at"] + 6):
        (tmp_path / "corpus.bin").write_bytes(flipped(blob, at))
        r = run(cli, tmp_path, "d", str(tmp_path / "corpus.bin"), W3_MODEL=model)
        assert r.returncode != 0 and "header" in r.stderr, r.stderr
        assert not (tmp_path / "corpus.orig").exists()
    # the intact file again
    (tmp_path / "corpus.bin").write_bytes(blob)
    assert run(cli, tmp_path, "d", str(tmp_path / "corpus.bin"), W3_MODEL=model).returncode == 0
    assert (tmp_path / "corpus.orig").read_bytes() == data


def test_random_access_on_the_checked_container(cli, tmp_path):
    data = markov_text(3 * BS, seed=83) + mixed_bytes(BS + 99, seed=84)
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)
    assert run(cli, tmp_path, "c", str(f), W3_CHECK="1").returncode == 0
    blob = (tmp_path / "corpus.bin").read_bytes()
    c = parse(blob)
    assert c["version"] == 3
    part = tmp_path / "corpus.part"

    def extract(off, n):
        if part.exists():
            part.unlink()
        return run(cli, tmp_path, "r", str(tmp_path / "corpus.bin"), str(off), str(n))

    r = extract(BS - 10, BS + 30)
    assert r.returncode == 0 and part.read_bytes() == data[BS - 10:2 * BS + 20], r.stderr
    at = c["streams_at"] + sum(c["lens"][:2]) + c["lens"][2] // 2               # damage block 2
    (tmp_path / "corpus.bin").write_bytes(flipped(blob, at))
    r = extract(2 * BS + 5, 10)                                                  # its first bytes decode, the block is not intact
    assert r.returncode != 0 and "block 2 " in r.stderr and not part.exists(), r.stderr
    r = extract(BS - 10, BS + 30)
    assert r.returncode != 0 and "block 2 " in r.stderr and not part.exists(), r.stderr
    r = extract(3 * BS - 3, 50)                                                   # the last bytes of block 2, then block 3
    assert r.returncode != 0
    r = extract(3 * BS, 500)
    assert r.returncode == 0 and part.read_bytes() == data[3 * BS:3 * BS + 500], r.stderr
    r = extract(100, BS)
    assert r.returncode == 0 and part.read_bytes() == data[100:100 + BS], r.stderr
    (tmp_path / "corpus.bin").write_bytes(flipped(blob, c["crc_at"] + 1))
    r = extract(100, 10)
    assert r.returncode != 0 and "header" in r.stderr


def test_random_access_refuses_version_4(cli, tmp_path):
    f = tmp_path / "corpus.txt"
    f.write_bytes(markov_text(BS + 500, seed=85))
    assert run(cli, tmp_path, "c", str(f), W3_MODEL="aoh:9,16", W3_CHECK="1").returncode == 0
    assert (tmp_path / "corpus.bin").read_bytes()[4] == 4
    r = run(cli, tmp_path, "r", str(tmp_path / "corpus.bin"), "10", "100")
    assert r.returncode != 0 and "random access is not implemented" in r.stderr
