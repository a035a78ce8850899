"""CPU truth of the AC-over-Huffman coder (bin/ac-over-huffman/main.rs:69-89) for the tests, composed from the oracle's own parts
(package_merge, canonical, OrderN, ArithmeticCoder, the byte and counting sinks) — a restatement, not the reference.

Two forms with the same results: the per-bit Python composition (about 3 us per coded bit: fine for small cases) and the C helper
tests/host/aoh_ref.c over threads, built on demand with the C compiler into a directory of the caller's (tmp_path).  Where no C
compiler is found the entry points below fall back to the Python composition: slower, never a skip."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "aoh_ref.c")
NTHREADS = 16


def code_table(orc, data, huffman_size):
    """(codes[256], lens[256]) as the driver builds them (:74-76): histogram -> package_merge -> canonical"""
    counts = np.bincount(np.frombuffer(bytes(data), dtype=np.uint8), minlength=256).tolist()
    pairs = orc.canonical(orc.package_merge(counts, huffman_size))
    return [c for c, _ in pairs], [l for _, l in pairs]


def identity_table():
    return list(range(256)), [8] * 256


def _blocks(data, block_size):
    return [data[i:i + block_size] for i in range(0, len(data), block_size)]


# ---- per-bit composition through pyoracle ---------------------------------------------------------------------------------------
def py_encode_block(orc, codes, lens, ctx_bits, block, stats=False):
    """one block: (stream bytes, ACStats bit count before flush)"""
    ac = orc.ArithmeticCoder.new_coder()
    model = orc.OrderN(ctx_bits, 0)
    w = orc.ACStats() if stats else orc.ACWriter()
    for byte in block:
        code, ln = codes[byte], lens[byte]
        for i in range(ln - 1, -1, -1):
            p = model.predict()
            bit = (code >> i) & 1
            model.update(bit)
            ac.encode(bit, p, w)
    if stats:
        return b"", int(w.s.bit_count)
    ac.flush(w)
    return w.bytes(), None


def py_encode_blocks(orc, codes, lens, ctx_bits, data, block_size):
    streams = [py_encode_block(orc, codes, lens, ctx_bits, blk)[0] for blk in _blocks(data, block_size)]
    return b"".join(streams), np.array([len(s) for s in streams], dtype=np.uint32)


def py_stats_bits(orc, codes, lens, ctx_bits, data, block_size):
    return np.array([py_encode_block(orc, codes, lens, ctx_bits, blk, stats=True)[1] for blk in _blocks(data, block_size)], dtype=np.uint64)


def py_decode_blocks(orc, codes, lens, ctx_bits, comp, block_lens, block_size, orig_len):
    sym = {(codes[s], lens[s]): s for s in range(256) if lens[s]}
    out = bytearray()
    off = 0
    for b, cl in enumerate(block_lens):
        n = min(block_size, orig_len - b * block_size)
        rd = orc.ACReader(bytes(comp[off:off + int(cl)]))
        off += int(cl)
        ac = orc.ArithmeticCoder.new_decoder(rd)
        model = orc.OrderN(ctx_bits, 0)
        for _ in range(n):
            code, ln = 0, 0
            while (code, ln) not in sym and ln < 16:
                p = model.predict()
                bit = ac.decode(p, rd)
                model.update(bit)
                code, ln = code << 1 | bit, ln + 1
            out.append(sym.get((code, ln), 0))
    return bytes(out)


# ---- the C helper ---------------------------------------------------------------------------------------------------------------
_cache = {}


def c_lib(build_dir):
    """tests/host/aoh_ref.c as a shared library in build_dir, or None without a C compiler"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        return None
    key = str(build_dir)
    if key not in _cache:
        so = os.path.join(key, "libaoh_ref.so")
        subprocess.check_call([cc, "-O2", "-std=c11", "-D_GNU_SOURCE", "-shared", "-fPIC", "-I", os.path.join(ROOT, "oracle"), "-o", so, SRC,
                               os.path.join(ROOT, "oracle", "w3_oracle.c"), "-lpthread", "-lm"])
        lib = C.CDLL(so)
        vp, sz = C.c_void_p, C.c_size_t
        lib.aoh_encode_blocks.argtypes = [vp, vp, C.c_uint8, vp, sz, sz, vp, sz, C.POINTER(sz), vp, C.c_int]
        lib.aoh_stats_bits.argtypes = [vp, vp, C.c_uint8, vp, sz, sz, vp, C.c_int]
        lib.aoh_stats_bits.restype = None
        lib.aoh_decode_blocks.argtypes = [vp, vp, C.c_uint8, vp, vp, sz, sz, vp, C.c_int]
        lib.aoh_decode_blocks.restype = None
        _cache[key] = lib
    return _cache[key]


def _tab(codes, lens):
    return np.array(codes, dtype=np.uint16), np.array(lens, dtype=np.uint8)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def encode_blocks(orc, build_dir, codes, lens, ctx_bits, data, block_size):
    """-> (streams: bytes, block_lens: np.uint32[nb])"""
    lib = c_lib(build_dir)
    if lib is None:
        return py_encode_blocks(orc, codes, lens, ctx_bits, data, block_size)
    c, l = _tab(codes, lens)
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    nb = (len(a) + block_size - 1) // block_size
    cap = 2 * len(a) + 64 * nb + 64
    while True:
        out = np.empty(max(cap, 1), dtype=np.uint8)
        bl = np.zeros(max(nb, 1), dtype=np.uint32)
        need = C.c_size_t()
        rc = lib.aoh_encode_blocks(_p(c), _p(l), ctx_bits, _p(a), len(a), block_size, _p(out), cap, C.byref(need), _p(bl), NTHREADS)
        if rc == -2:
            cap = need.value
            continue
        assert rc == 0
        return out[:need.value].tobytes(), bl[:nb]


def stats_bits(orc, build_dir, codes, lens, ctx_bits, data, block_size):
    """-> np.uint64[nb] ACStats bit counts"""
    lib = c_lib(build_dir)
    if lib is None:
        return py_stats_bits(orc, codes, lens, ctx_bits, data, block_size)
    c, l = _tab(codes, lens)
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    nb = (len(a) + block_size - 1) // block_size
    bits = np.zeros(max(nb, 1), dtype=np.uint64)
    lib.aoh_stats_bits(_p(c), _p(l), ctx_bits, _p(a), len(a), block_size, _p(bits), NTHREADS)
    return bits[:nb]


def decode_blocks(orc, build_dir, codes, lens, ctx_bits, comp, block_lens, block_size, orig_len):
    lib = c_lib(build_dir)
    if lib is None:
        return py_decode_blocks(orc, codes, lens, ctx_bits, comp, block_lens, block_size, orig_len)
    c, l = _tab(codes, lens)
    a = np.frombuffer(bytes(comp), dtype=np.uint8)
    bl = np.ascontiguousarray(block_lens, dtype=np.uint32)
    out = np.empty(max(orig_len, 1), dtype=np.uint8)
    lib.aoh_decode_blocks(_p(c), _p(l), ctx_bits, _p(a), _p(bl), block_size, orig_len, _p(out), NTHREADS)
    return out[:orig_len].tobytes()
