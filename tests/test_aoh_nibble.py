"""The nibble logic of the sixteen-lanes-per-job decoder of AC over Huffman (weath3rb0i_amd/csrc/w3_aoh_nibble.h, the plain-C++ part
of k_aoh_decode_spec) on the CPU: tests/host/aoh_nibble.cpp simulates a row of the kernel with it — 15 snapshot loads per nibble from
a table array, four steps with forwarding, last-writer stores after the nibble — over the oracle's Counter and arithmetic decoder, on
the streams of tests/aoh_ref.py.  The result must be the encoder's input; on a stream that is not one of ours, the serial decoder's
output.  The hazard the two rules exist for (two steps of one nibble on one context) is counted, so that it cannot be absent, and two
deliberately wrong variants of the simulation must fail where it is everywhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import aoh_ref
from tests.synth import markov_text, mixed_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "aoh_nibble.cpp")
CTX_BITS = [1, 2, 3, 8, 16, 24]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or shutil.which("gcc") is None, reason="gcc / g++ not found")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("aoh_nibble")


@pytest.fixture(scope="module")
def sim(build_dir):
    obj, so = str(build_dir / "w3_oracle.o"), str(build_dir / "libaoh_nibble.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-D_GNU_SOURCE", "-fPIC", "-c", "-I", os.path.join(ROOT, "oracle"), "-o", obj,
                           os.path.join(ROOT, "oracle", "w3_oracle.c")])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "oracle"), "-o", so, SRC, obj,
                           "-lpthread", "-lm"])
    lib = C.CDLL(so)
    vp, sz = C.c_void_p, C.c_size_t
    lib.aoh_nibble_decode.argtypes = [vp, vp, C.c_uint8, vp, sz, sz, vp, C.c_int, C.POINTER(C.c_uint64 * 3), C.POINTER(C.c_uint64)]

    def run(codes, lens, cb, stream, job_len, variant=0, dst=0):
        """-> (decoded bytes, nibbles, full nibbles, full nibbles with two equal path contexts); dst: the output's offset from a 16-byte
        boundary — the bytes around the job's must stay untouched, and all but the unaligned ends must leave as aligned words"""
        c, l = np.array(codes, dtype=np.uint16), np.array(lens, dtype=np.uint8)
        s = np.frombuffer(bytes(stream), dtype=np.uint8)
        raw = np.full(job_len + 48, 0xEE, dtype=np.uint8)
        at = (-raw.ctypes.data) % 16 + dst
        cnt, words = (C.c_uint64 * 3)(), C.c_uint64()
        rc = lib.aoh_nibble_decode(c.ctypes.data_as(vp), l.ctypes.data_as(vp), cb, s.ctypes.data_as(vp), len(s), job_len, vp(raw.ctypes.data + at),
                                   variant, C.byref(cnt), C.byref(words))
        assert rc == 0, "a path node's snapshot context is not the step's context (-1), or a misaligned word store (-2): %d" % rc
        assert (raw[:at] == 0xEE).all() and (raw[at + job_len:] == 0xEE).all()
        head = min((-dst) % 4, job_len)
        assert words.value == (job_len - head) // 4
        return raw[at:at + job_len].tobytes(), int(cnt[0]), int(cnt[1]), int(cnt[2])

    return run


def _streams(comp, lens):
    offs = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
    return [bytes(comp[offs[b]:offs[b + 1]]) for b in range(len(lens))]


def _check(sim, oracle, build_dir, codes, lens, cb, data, bs):
    """every block's stream at job lengths 1, 2, block - 1 and block; -> (full nibbles, those with two equal path contexts) of the whole-block jobs"""
    comp, bl = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, cb, data, bs)
    full = equal = 0
    for b, stream in enumerate(_streams(comp, bl)):
        blk = data[b * bs:(b + 1) * bs]
        for job in sorted({1, 2, len(blk) - 1, len(blk)} - {0}):
            got, _, f, e = sim(codes, lens, cb, stream, job, dst=(b + job) % 5)
            assert got == blk[:job], (cb, b, job)
            if job == len(blk):
                full, equal = full + f, equal + e
    return full, equal


@pytest.mark.parametrize("hsize", [6, 9, 13])
def test_row_simulation_decodes_text(sim, oracle, build_dir, hsize):
    data = markov_text(20000, seed=41)
    codes, lens = aoh_ref.code_table(oracle, data, hsize)
    for cb in CTX_BITS:
        full, equal = _check(sim, oracle, build_dir, codes, lens, cb, data, 5000)
        assert full > 0
        if cb == 1:
            assert equal == full          # four steps over two contexts
        if cb <= 8:
            assert equal > 0              # the hazard is there: the rules are exercised


def test_row_simulation_decodes_mixed_bytes(sim, oracle, build_dir):
    data = mixed_bytes(20000, seed=43)
    codes, lens = aoh_ref.code_table(oracle, data, 9)
    for cb in CTX_BITS:
        _check(sim, oracle, build_dir, codes, lens, cb, data, 5000)


def test_all_zero_bit_string(sim, oracle, build_dir):
    """the two-symbol table: an all-zero bit string, one context beyond 65,535 hits, four symbols per nibble — every full nibble has
    one context four times, whatever ctx_bits"""
    data = b"a" * 70000 + b"b"
    codes, lens = aoh_ref.code_table(oracle, data, 12)
    assert (codes[97], lens[97], codes[98], lens[98]) == (0, 1, 1, 1)
    for cb in CTX_BITS:
        full, equal = _check(sim, oracle, build_dir, codes, lens, cb, data, 1 << 17)
        assert full == 17500 and equal == full


def test_foreign_stream_equals_the_serial_decoder(sim, oracle, build_dir):
    """random bytes are a stream too: the row decodes them to what the serial decoder does"""
    data = markov_text(20000, seed=41)
    rng = np.random.default_rng(9)
    for hsize, cb in ((9, 8), (13, 16), (6, 3)):
        codes, lens = aoh_ref.code_table(oracle, data, hsize)
        garbage = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
        n = 1500
        want = aoh_ref.decode_blocks(oracle, build_dir, codes, lens, cb, garbage, np.array([len(garbage)], dtype=np.uint32), n, n)
        assert sim(codes, lens, cb, garbage, n)[0] == want


@pytest.mark.parametrize("variant", [1, 2], ids=["every_path_node_stores", "no_forwarding"])
def test_the_simulation_catches_a_missing_rule(sim, oracle, build_dir, variant):
    """The simulation without the last-writer rule (every path node stores; within one nibble the stores land in descending step order,
    which the hardware may do) or without forwarding must NOT decode the all-zero case — otherwise the tests above prove nothing."""
    data = b"a" * 70000 + b"b"
    codes, lens = aoh_ref.code_table(oracle, data, 12)
    comp, bl = aoh_ref.encode_blocks(oracle, build_dir, codes, lens, 8, data, 1 << 17)
    assert sim(codes, lens, 8, comp, len(data), 0)[0] == data
    assert sim(codes, lens, 8, comp, len(data), variant)[0] != data
