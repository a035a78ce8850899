"""Inputs steered into long pending-bit (E3 / underflow) runs of the 32-bit binary arithmetic coder (arithmetic_coder.rs:41-65), built
on the CPU with the oracle alone: test infrastructure, no device code.

Every bit of an input is free.  With the coder at (x1, x2) and the model's next probability p, the step's split point is
xmid = lerp(x1, x2, p).  Bit 1 keeps [x1, xmid], bit 0 keeps [xmid + 1, x2]: taking bit 1 iff xmid >= 2^31 keeps the interval astride
the midpoint, and every further halving of the range is one more pending bit (ACWriter::rev_bits).  Taking the OTHER bit releases the
run: first bit 1 then zeros when the interval lands above the midpoint (released by bit 0 — the carry case of the slot accumulators
in w3_coder.h), 0 then ones when it lands below (released by bit 1).

All functions are seeded and deterministic.  Each builds its data block by block with a fresh model and coder per block, as
encode_blocks does, and returns (bytes, Trace): the trace is read off the oracle's sink while the data is being made."""
import ctypes as C

import numpy as np

from oracle import pyoracle as orc
from tests.synth import markov_text

MID = 0x80000000
_predict = orc.lib.w3o_model_predict
_update = orc.lib.w3o_model_update
_encode = orc.lib.w3o_ac_encode


class Trace:
    """What the oracle's sink saw, per block: runs = resolved runs as (length, first bit); end_pending = the pending count at the
    block's end, before the flush; longest = the longest run, resolved or not; handback = a step was coded with 64 or more bits
    pending (a run no 64-bit slot accumulator can hold: every fast coder has to hand the block back); streams = the block's stream."""

    def __init__(self, block_size):
        self.block_size = block_size
        self.runs, self.end_pending, self.longest, self.handback, self.streams = [], [], [], [], []

    def add(self, other):
        for k in ("runs", "end_pending", "longest", "handback", "streams"):
            getattr(self, k).extend(getattr(other, k))

    @property
    def nblocks(self):
        return len(self.streams)

    def lens(self):
        return [len(s) for s in self.streams]

    def stream(self):
        return b"".join(self.streams)

    def run_lengths(self, first_bit):
        return {n for rs in self.runs for n, b in rs if b == first_bit}


class _Block:
    """One block's fresh predictor, coder and byte sink, stepped a bit at a time: look() then put(bit)."""

    def __init__(self, model):
        self.model = model
        self.ac = orc.ArithmeticCoder.new_coder()
        self.w = orc.ACWriter()
        self.s = self.w.s
        self._ac, self._s, self._m = C.byref(self.ac.ac), C.byref(self.s), model.ptr
        self.runs, self.longest, self.handback = [], 0, False
        self.p = self.xmid = None

    def look(self):
        """predicts the next step; -> the bit that keeps the interval astride the midpoint (and self.xmid)"""
        p = self.p = _predict(self._m)
        a = self.ac.ac
        x1 = a.x1
        self.xmid = x1 + (((a.x2 - x1) * ((p << 16) if p else 1)) >> 32)   # arithmetic_coder.rs:109-119
        return 1 if self.xmid >= MID else 0

    def put(self, bit):
        rev = self.s.rev_bits
        if rev >= 64:
            self.handback = True
        a = self.ac.ac
        nx1, nx2 = (a.x1, self.xmid) if bit else (self.xmid + 1, a.x2)
        if rev and not ((nx1 ^ nx2) >> 31):     # the first renormalisation loop runs: its first write_bit resolves the run
            self.runs.append((rev, nx1 >> 31))
        _update(self._m, bit)
        _encode(self._ac, bit, self.p, self._s)
        r = self.s.rev_bits
        if r > self.longest:
            self.longest = r

    @property
    def pending(self):
        return self.s.rev_bits

    def after(self, bit):
        """the pending count that put(bit) would leave (arithmetic_coder.rs:45-62 on a copy of the coder's state)"""
        a, rev = self.ac.ac, self.s.rev_bits
        x1, x2 = (a.x1, self.xmid) if bit else (self.xmid + 1, a.x2)
        while not ((x1 ^ x2) >> 31):
            rev, x1, x2 = 0, (x1 << 1) & 0xFFFFFFFF, (x2 << 1 | 1) & 0xFFFFFFFF
        while x1 >= 0x40000000 and x2 < 0xC0000000:
            rev, x1, x2 = rev + 1, (x1 << 1) & 0x7FFFFFFF, (x2 << 1 | 0x80000001) & 0xFFFFFFFF
        return rev


class _Bytes:
    """Bits to bytes, MSB first, blocks of block_size bytes."""

    def __init__(self, new_model, block_size):
        self.new, self.bs = new_model, block_size
        self.out, self.tr = bytearray(), Trace(block_size)
        self.blk, self.filled = None, 0
        self.cur = self.nbits = 0
        self.model = None

    def _fresh(self):
        """one model per builder, reset for every block as the oracle's encode_blocks does (building a model can cost milliseconds)"""
        if self.model is None:
            self.model = self.new()
        else:
            self.model.reset()
        return self.model

    @property
    def partial(self):
        return self.nbits != 0

    def block(self):
        if self.blk is None:
            self.blk, self.filled = _Block(self._fresh()), 0
        return self.blk

    def bits_left(self):
        return (self.bs - self.filled) * 8 - self.nbits

    def _symbol(self, bit):
        self.cur, self.nbits = self.cur << 1 | bit, self.nbits + 1
        if self.nbits < 8:
            return None
        v, self.cur, self.nbits = self.cur, 0, 0
        return v

    def put(self, bit):
        self.blk.put(bit)
        v = self._symbol(bit)
        if v is not None:
            self.out.append(v)
            self.filled += 1
            if self.filled == self.bs:
                self.close()

    def put_byte(self, v):
        for j in range(7, -1, -1):
            self.block().look()
            self.put((v >> j) & 1)

    def close(self):
        b, t = self.blk, self.tr
        t.runs.append(b.runs)
        t.end_pending.append(b.pending)
        t.longest.append(b.longest)
        t.handback.append(b.handback)
        b.ac.flush(b.w)
        t.streams.append(b.w.bytes())
        self.blk = None

    def done(self):
        assert not self.partial
        if self.blk is not None:
            self.close()
        return bytes(self.out), self.tr

    def runs_so_far(self):
        return [r for rs in self.tr.runs for r in rs] + (self.blk.runs if self.blk is not None else [])


class _Huff(_Bytes):
    """Bits to bytes through a complete canonical code (codes not bit-reversed: the first coded bit is the code's top bit)."""

    def __init__(self, codes, lens, ctx_bits, block_size):
        super().__init__(lambda: orc.OrderN(ctx_bits, 0), block_size)
        self.sym = {(codes[s], lens[s]): s for s in range(256) if lens[s]}
        assert sum(2.0 ** -n for _, n in self.sym) == 1.0, "the code is not complete: not every bit string is a symbol sequence"

    def _symbol(self, bit):
        self.cur, self.nbits = self.cur << 1 | bit, self.nbits + 1
        v = self.sym.get((self.cur, self.nbits))
        if v is not None:
            self.cur = self.nbits = 0
        return v


# ---- strategies over a builder ----------------------------------------------------------------------------------------------------
def _hold(B, nbytes):
    while len(B.out) < nbytes or B.partial:
        B.put(B.block().look())


def _filler(B, rng, nbits):
    for _ in range(nbits):
        B.block().look()
        B.put(int(rng.integers(0, 2)))


def _runs(B, targets, gap_bytes, rng, cap=None):
    """cap: a run that has reached this many pending bits is released whatever its polarity"""
    for length, first_bit in targets:
        while True:
            blk = B.block()
            hb = blk.look()
            # taking the other bit now resolves the run with first bit hb (above the midpoint after bit 0, below after bit 1)
            if (blk.pending >= length and hb == first_bit and blk.xmid != MID - 1) or (cap is not None and blk.pending >= cap):
                B.put(1 - hb)
                break
            B.put(hb)
        _filler(B, rng, 8 * gap_bytes)
    while B.partial:
        _filler(B, rng, 1)


def _missing(runs, want):
    have = set(runs)
    return [(n, b) for n, b, tol in want if not any((m, b) in have for m in range(n - tol, n + tol + 1))]


SMALL = [(n, b, 0) for n in range(1, 81) for b in (0, 1)]
KEPT = [(n, b, 0) for n in range(1, 38) for b in (0, 1)]    # (a slot accumulator holds 38 pending ones whatever is above the slot: w3_coder.h)
LARGE = [(n, b, 2) for n in (127, 128, 129, 255, 256, 257, 1000, 4096) for b in (0, 1)]


def _coverage(B, gap_bytes, rng, want, passes=40, cap=None):
    """runs() over `want` ((length, first bit, tolerance) triples), again over what a pass missed, until every one has occurred"""
    for _ in range(passes):
        missing = _missing(B.runs_so_far(), want)
        if not missing:
            return
        # (a step can add several pending bits: aim at the low end of a tolerance window)
        tol = {(n, b): t for n, b, t in want}
        _runs(B, [(n - tol[(n, b)], b) for n, b in missing], gap_bytes, rng, cap)
    raise AssertionError("run lengths still missing after %d passes: %r" % (passes, _missing(B.runs_so_far(), want)))


# ---- byte models ------------------------------------------------------------------------------------------------------------------
def hold(model_factory, nbytes, block_size):
    """holds the midpoint from every block's first bit: each block is ONE pending run that only the flush resolves"""
    B = _Bytes(model_factory, block_size)
    _hold(B, nbytes)
    return B.done()


def runs(model_factory, targets, gap_bytes, block_size, seed=1):
    """per (length, first bit) target: holds until that many bits are pending and the wanted polarity is on offer (else one more step),
    releases, codes gap_bytes of random filler"""
    B = _Bytes(model_factory, block_size)
    _runs(B, targets, gap_bytes, np.random.default_rng(seed))
    return B.done()


def run_coverage(model_factory, block_size, gap_bytes=2, seed=1, want=None, cap=None):
    """runs() repeated over the targets a pass missed until every exact length 1..80, and 127 / 128 / 129, 255 / 256 / 257, 1,000 and 4,096
    within 2, has occurred with both first bits (or every (length, first bit, tolerance) of `want`)"""
    B = _Bytes(model_factory, block_size)
    _coverage(B, gap_bytes, np.random.default_rng(seed), LARGE + SMALL if want is None else want, cap=cap)
    return B.done()


def block_ends(model_factory, block_size, nblocks, seed=3, top=90, attempts=8):
    """blocks of random filler that hold the midpoint over their last steps, aimed at the end-of-block pending counts 0..top, the least
    seen first.  A step can add no pending bit or several, so the last steps choose between holding and releasing by the count each
    would leave, and while counts are still missing a block that ends on one already seen is remade with other filler, `attempts`
    times at most."""
    tr, out = Trace(block_size), bytearray()
    seen = [0] * (top + 1)
    nbits = block_size * 8
    model = model_factory()
    for k in range(nblocks):
        low = min(seen)
        want = seen.index(low)
        best = None
        for attempt in range(attempts):
            rng = np.random.default_rng([seed, k, attempt])
            B = _Bytes(lambda: model, block_size)
            model.reset()
            _filler(B, rng, max(0, nbits - want - 6))
            while B.blk is not None:      # the last steps: whichever bit brings (pending + steps left) nearer to the count, the hold bit first
                blk, left = B.blk, B.bits_left() - 1
                hb = blk.look()
                B.put(hb if abs(blk.after(hb) + left - want) <= abs(blk.after(1 - hb) + left - want) else 1 - hb)
            data, t = B.done()
            got = t.end_pending[0]
            if best is None or abs(got - want) < abs(best[2] - want):
                best = (data, t, got)
            if low or (got <= top and not seen[got]):     # a count not seen yet; once all have been seen, any
                best = (data, t, got)
                break
        data, t, got = best
        if got <= top:
            seen[got] += 1
        out += data
        tr.add(t)
    return bytes(out), tr


def mixed(model_factory, block_size, nblocks, tail, seed=5):
    """nblocks blocks, the last one of `tail` bytes.  Every third block (0, 3, ...) is text, then a held run of 64 or more bits that is
    released, then text to the block's end; every other block is plain text."""
    rng = np.random.default_rng(seed)
    text = markov_text(block_size * nblocks, seed=seed + 100)
    B = _Bytes(model_factory, block_size)
    for k in range(nblocks):
        n = tail if k == nblocks - 1 else block_size
        src = text[k * block_size:k * block_size + n]
        if k % 3:
            for v in src:
                B.put_byte(v)
            continue
        prefix = 0 if k == 0 else int(rng.integers(0, min(96, n // 3)))
        length = 64 + int(rng.integers(0, 120)) if k % 5 else int(rng.integers(300, 1200))
        for v in src[:prefix]:
            B.put_byte(v)
        while True:
            blk = B.block()
            hb = blk.look()
            if blk.pending >= length and blk.xmid != MID - 1:
                B.put(1 - hb)
                break
            B.put(hb)
        while B.partial:
            _filler(B, rng, 1)
        for v in src[B.filled:]:
            B.put_byte(v)
    return B.done()


def anti(model_factory, nbytes, block_size):
    """always the less probable bit: every block's stream is longer than the block"""
    B = _Bytes(model_factory, block_size)
    while len(B.out) < nbytes:
        blk = B.block()
        blk.look()
        B.put(0 if blk.p >= 32768 else 1)
    return B.done()


def replay(model_factory, data, block_size):
    """the trace of given bytes"""
    B = _Bytes(model_factory, block_size)
    for v in data:
        B.put_byte(v)
    return B.done()[1]


# ---- AC over Huffman: OrderN(ctx_bits, 0) over the bit string of the bytes' codes (bin/ac-over-huffman/main.rs:69-89) -----------------
def aoh_hold(codes, lens, ctx_bits, nbytes, block_size):
    """hold() over the Huffman bit string; the last symbol is finished with the bits the hold asks for"""
    B = _Huff(codes, lens, ctx_bits, block_size)
    _hold(B, nbytes)
    return B.done()


def aoh_runs(codes, lens, ctx_bits, targets, gap_bytes, block_size, seed=1):
    B = _Huff(codes, lens, ctx_bits, block_size)
    _runs(B, targets, gap_bytes, np.random.default_rng(seed))
    return B.done()


def aoh_run_coverage(codes, lens, ctx_bits, block_size, gap_bytes=2, seed=1, want=None):
    B = _Huff(codes, lens, ctx_bits, block_size)
    _coverage(B, gap_bytes, np.random.default_rng(seed), LARGE + SMALL if want is None else want)
    return B.done()


# ---- the inputs of tests/test_steer_cpu.py and tests/test_gpu_steer.py, made once per session ----------------------------------------------
COUNTER_MODELS = ["order0", "best01", "best012", "main_default", "best_ac_wide"]      # names of tests/test_gpu_parity.py's pair()
CM_MODELS = ["o012_apm", "apm_chain4", "slot_mix", "full_cm_small_tables"]            # names of tests/test_gpu_cm.py's pair()
AOH_CTX_BITS = [8, 16, 25]
AOH_HSIZE = 9
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def counter_input(name, factory, kind):
    """(data, trace) of one of a Counter model's inputs, steered under that very model (`factory`: fresh oracle model).
    coverage: every run length of LARGE + SMALL, block size 8192 (a fast coder hands such a block back at its first long run).  kept:
    every run length 1..37 in blocks of 128 bytes in which no run grows past 38, so that no coder hands any of them back.  ends: 192 blocks of 48 bytes, every end-of-block pending count 0..90.
    hold: one block of 16 KiB that is a single run plus a ragged second one.  mixed: 130 blocks of 512 bytes (the last one 200), every
    third with a run of 64 or more.  anti: 1 KiB blocks that expand, ragged tail."""
    make = {"coverage": lambda: run_coverage(factory, 8192), "kept": lambda: run_coverage(factory, 128, want=KEPT, cap=37),
            "ends": lambda: block_ends(factory, 48, 192),
            "hold": lambda: hold(factory, 16384 + 1000, 16384), "mixed": lambda: mixed(factory, 512, 130, 200),
            "anti": lambda: anti(factory, 4096 + 300, 1024)}[kind]
    return _once((name, kind), make)


BLOCK_SIZE = {"coverage": 8192, "kept": 128, "ends": 48, "hold": 16384, "mixed": 512, "anti": 1024}


def cm_input(name, factory, kind):
    """coverage and kept as above; ends: 200 blocks of 48 bytes"""
    make = {"coverage": lambda: run_coverage(factory, 8192), "kept": lambda: run_coverage(factory, 128, want=KEPT, cap=37),
            "ends": lambda: block_ends(factory, 48, 200)}[kind]
    return _once((name, kind), make)


def aoh_table():
    """(codes, lens): the driver's table (histogram -> package_merge -> canonical) of Markov text at huffman_size 9"""
    from tests import aoh_ref
    return _once("aoh_table", lambda: aoh_ref.code_table(orc, markov_text(40000, seed=61), AOH_HSIZE))


def aoh_input(ctx_bits, kind):
    """runs: every run length of LARGE + SMALL over the Huffman bit string, blocks of 4096 bytes.  hold: one block of 28 KiB that is a
    single run (a Huffman symbol takes fewer steps than a byte) plus a ragged second one."""
    codes, lens = aoh_table()
    make = {"runs": lambda: aoh_run_coverage(codes, lens, ctx_bits, 4096), "hold": lambda: aoh_hold(codes, lens, ctx_bits, 28672 + 700, 28672)}[kind]
    return _once(("aoh", ctx_bits, kind), make)


AOH_BLOCK_SIZE = {"runs": 4096, "hold": 28672}
