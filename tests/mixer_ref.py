"""CPU truth of the logistic mixer node (W3_NODE_MIX: include/w3hip.h) for the tests, in plain Python integers and
composed from oracle parts — a restatement, not the reference (which has no such node): the leaves' streams from pyoracle.predict_all
per leaf, the step below, APM stages behind it from tests/apm_census.stage, the oracle's ArithmeticCoder with its byte and counting sinks,
and its decoder for the round trip (there the same model runs bit by bit: `Incremental`).

The step.  State w[S][N] int32, S = 1 (ONE) or 256 (ORDER0), every weight 65536 // N at the block start; WMAX = 2^20 - 1.  Step 8 i + j is
bit j (most significant first) of byte i; the ORDER0 row is c0 = (1 << j) | (byte >> (8 - j)), taken before the bit.
    s_i = stretch[p_i >> 4];  dot = sum((w_i * s_i) >> 8);  d = clamp(dot >> 8, -2047, 2047);  p = squash[d + 2047]
    err = (bit << 16) - p;    w_i = clamp(w_i + ((s_i * err + (1 << (rate - 1))) >> rate), -WMAX, WMAX)
Python's >> on negative integers is the arithmetic shift the definition asks for.  Both products and the sum are asserted to fit int32 at
every step."""
import collections

from tests import apm_census as ac

ONE, ORDER0 = 0, 1
WMAX = (1 << 20) - 1
I32 = 1 << 31

MUTANTS = ["no_rounding", "truncating_shift", "clamp_at_2_20", "err_from_65535", "row_after_bit", "update_before_predict", "one_shift_16"]
STATES = ["d_lo", "d_hi", "w_max", "w_min", "w_negative"]


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def predict_d(w, s, mutant=None):
    if mutant == "one_shift_16":
        tot = sum(wi * si for wi, si in zip(w, s))
        return _clamp(tot >> 16, -2047, 2047)
    dot = 0
    for wi, si in zip(w, s):
        assert -I32 <= wi * si < I32
        dot += (wi * si) >> 8
    assert -I32 <= dot < I32
    return _clamp(dot >> 8, -2047, 2047)


def train(w, s, bit, p, rate, mutant=None):
    err = (65535 if bit else 0) - p if mutant == "err_from_65535" else (bit << 16) - p
    rnd = 0 if mutant == "no_rounding" else 1 << (rate - 1)
    wmax = 1 << 20 if mutant == "clamp_at_2_20" else WMAX
    for i, si in enumerate(s):
        v = si * err + rnd
        assert -I32 <= v < I32
        if mutant == "truncating_shift":
            dv = -((-v) >> rate) if v < 0 else v >> rate
        else:
            dv = v >> rate
        w[i] = _clamp(w[i] + dv, -wmax, wmax)


def mix(streams, block, select=ORDER0, rate=14, mutant=None, states=None, rows=None):
    """the mixer over the leaves' streams of one block -> its output stream (list of 8 len ints).  states: a Counter that receives the
    names of STATES reached; rows: a set that receives the ORDER0 rows visited."""
    n = len(streams)
    assert 2 <= n <= 8 and 4 <= rate <= 20 and select in (ONE, ORDER0)
    w = [[65536 // n] * n for _ in range(256 if select == ORDER0 else 1)]
    out = []
    t = 0
    for byte in bytes(block):
        for j in range(8):
            bit = (byte >> (7 - j)) & 1
            c0 = (1 << j) | (byte >> (8 - j))
            if mutant == "row_after_bit":
                c0 = (c0 << 1 | bit) if j < 7 else 1
            ww = w[c0 if select == ORDER0 else 0]
            s = [ac.STRETCH[p[t] >> 4] for p in streams]
            d = predict_d(ww, s, mutant)
            p = ac.SQUASH[d + 2047]
            train(ww, s, bit, p, rate, mutant)
            if mutant == "update_before_predict":
                p = ac.SQUASH[predict_d(ww, s, mutant) + 2047]
            out.append(p)
            if states is not None:
                if d == -2047:
                    states["d_lo"] += 1
                if d == 2047:
                    states["d_hi"] += 1
                for wi in ww:
                    if wi == WMAX:
                        states["w_max"] += 1
                    if wi == -WMAX:
                        states["w_min"] += 1
                    if wi < 0:
                        states["w_negative"] += 1
            if rows is not None:
                rows.add(c0)
            t += 1
    return out


# ---- leaves: one description, two builders (the oracle's model, the package's) ---------------------------------------------------------
# ("o0",) ("o1",) ("on", bits, align) ("ac", bits, align, max_bits) = OrderNEntropy over ACHistory(max_bits, for_book1) ("slot", order, log_cells)
def orc_leaf(orc, leaf):
    k = leaf[0]
    if k == "o0":
        return orc.Order0()
    if k == "o1":
        return orc.Order1()
    if k == "on":
        return orc.OrderN(leaf[1], leaf[2])
    if k == "ac":
        return orc.OrderNEntropy(leaf[1], leaf[2], orc.ACHistory(leaf[3], orc.StationaryModel.for_book1()))
    assert k == "slot"
    return orc.SlotModel(leaf[1], leaf[2])


def w3_leaf(w3, leaf):
    k = leaf[0]
    if k == "o0":
        return w3.Order0()
    if k == "o1":
        return w3.Order1()
    if k == "on":
        return w3.OrderN(leaf[1], leaf[2])
    if k == "ac":
        return w3.OrderNEntropy(leaf[1], leaf[2], w3.ACHistory(leaf[3], w3.StationaryModel.for_book1()))
    return w3.SlotModel(leaf[1], leaf[2])


def w3_model(w3, leaves, select=ORDER0, rate=14, stages=()):
    m = w3.LogisticMixer([w3_leaf(w3, lf) for lf in leaves], select, rate)
    for kind, srate in stages:
        m = w3.APM(m, kind, srate)
    return m


def leaf_streams(orc, leaves, block):
    return [orc.predict_all(orc_leaf(orc, lf), bytes(block)).tolist() for lf in leaves]


def predict_block(orc, leaves, block, select=ORDER0, rate=14, stages=(), mutant=None):
    """the model's final stream of one block: mixer, then the APM stages ((kind, rate), ...) behind it"""
    p = mix(leaf_streams(orc, leaves, block), block, select, rate, mutant)
    for kind, srate in stages:
        p = ac.stage(p, bytes(block), kind, srate, with_kinds=False)[0]
    return p


def blocks_of(data, block_size):
    return [data[i:i + block_size] for i in range(0, len(data), block_size)]


def predict_blocks(orc, leaves, data, block_size, select=ORDER0, rate=14, stages=()):
    out = []
    for blk in blocks_of(data, block_size):
        out += predict_block(orc, leaves, blk, select, rate, stages)
    return out


def code_block(orc, p, block):
    """the oracle's coder over the stream p -> (stream bytes, ACStats bit count)"""
    enc, cnt = orc.ArithmeticCoder.new_coder(), orc.ArithmeticCoder.new_coder()
    w, st = orc.ACWriter(), orc.ACStats()
    t = 0
    for byte in bytes(block):
        for j in range(8):
            bit = (byte >> (7 - j)) & 1
            enc.encode(bit, p[t], w)
            cnt.encode(bit, p[t], st)
            t += 1
    bits = int(st.s.bit_count)
    enc.flush(w)
    return w.bytes(), bits


def encode_blocks(orc, leaves, data, block_size, select=ORDER0, rate=14, stages=()):
    """-> (streams: bytes, block_lens: list, block_bits: list)"""
    streams, lens, bits = [], [], []
    for blk in blocks_of(data, block_size):
        s, b = code_block(orc, predict_block(orc, leaves, blk, select, rate, stages), blk)
        streams.append(s)
        lens.append(len(s))
        bits.append(b)
    return b"".join(streams), lens, bits


# ---- the same model bit by bit (what a decoder runs) -----------------------------------------------------------------------------------
class _Apm:
    def __init__(self, kind, rate):
        self.kind, self.rate, self.t, self.idx = kind, rate, {}, None

    def _get(self, row, e):
        return self.t.get((row, e), ac.ROW_INIT[e])

    def pp(self, p, c0, c1):
        row = c0 | (c1 << 8) if self.kind == ac.ORDER1 else c0
        pos = (ac.STRETCH[p >> 4] + 2048) * 32
        j, w = pos >> 12, pos & 4095
        pa = (self._get(row, j) * (4096 - w) + self._get(row, j + 1) * w) >> 12
        self.idx = (row, j + (w >> 11))
        return _clamp((p + 3 * pa + 2) >> 2, 1, 65535)

    def update(self, bit):
        tv = self._get(*self.idx)
        self.t[self.idx] = tv + (((65535 if bit else 0) - tv) >> self.rate)


class Incremental:
    """predict() / update(bit) of the whole model, fresh for one block"""

    def __init__(self, orc, leaves, select=ORDER0, rate=14, stages=()):
        self.leaves = [orc_leaf(orc, lf) for lf in leaves]
        n = len(leaves)
        self.select, self.rate = select, rate
        self.w = [[65536 // n] * n for _ in range(256 if select == ORDER0 else 1)]
        self.apm = [_Apm(k, r) for k, r in stages]
        self.c0, self.c1 = 1, 0

    def predict(self):
        self.s = [ac.STRETCH[m.predict() >> 4] for m in self.leaves]
        self.ww = self.w[self.c0 if self.select == ORDER0 else 0]
        self.p = p = ac.SQUASH[predict_d(self.ww, self.s) + 2047]
        for a in self.apm:
            p = a.pp(p, self.c0, self.c1)
        return p

    def update(self, bit):
        train(self.ww, self.s, bit, self.p, self.rate)
        for a in self.apm:
            a.update(bit)
        for m in self.leaves:
            m.update(bit)
        self.c0 = self.c0 << 1 | bit
        if self.c0 >= 256:
            self.c1, self.c0 = self.c0 & 255, 1


def decode_blocks(orc, leaves, comp, block_lens, block_size, orig_len, select=ORDER0, rate=14, stages=()):
    out = bytearray()
    off = 0
    for b, cl in enumerate(block_lens):
        n = min(block_size, orig_len - b * block_size)
        rd = orc.ACReader(bytes(comp[off:off + int(cl)]))
        off += int(cl)
        dec = orc.ArithmeticCoder.new_decoder(rd)
        m = Incremental(orc, leaves, select, rate, stages)
        for _ in range(n):
            byte = 0
            for _j in range(8):
                bit = dec.decode(m.predict(), rd)
                m.update(bit)
                byte = byte << 1 | bit
            out.append(byte)
    return bytes(out)


# ---- directed inputs (at most 4 KiB): every clamp of the step at rate 4 over Order0 + Order1 --------------------------------------------
DIRECTED = {
    "zeros_then_ff00": bytes(2048) + bytes([0xFF, 0x00] * 1024),
    "runs_00_ff": bytes(1024) + b"\xff" * 1024 + bytes(1024) + b"\xff" * 1024,
    "zeros": bytes(4096),
    "ones": b"\xff" * 4096,
    "ramp": bytes(range(256)) * 2,
}
DIRECTED_LEAVES = (("o0",), ("o1",))


def reached(orc, name, select=ORDER0, rate=4):
    states, rows = collections.Counter(), set()
    mix(leaf_streams(orc, DIRECTED_LEAVES, DIRECTED[name]), DIRECTED[name], select, rate, states=states, rows=rows)
    return states, rows



def held_block(orc, leaves, nbytes, select=ORDER0, rate=14, stages=()):
    """a block steered into ONE pending-bit run (tests/steer.py's `hold` for this model): every bit is the one that keeps the coder's
    interval astride the midpoint under the model's own prediction -> (bytes, the longest run of pending bits)"""
    m = Incremental(orc, leaves, select, rate, stages)
    coder, w = orc.ArithmeticCoder.new_coder(), orc.ACWriter()
    out, longest = bytearray(), 0
    for _ in range(nbytes):
        byte = 0
        for _j in range(8):
            p = m.predict()
            x1, x2 = coder.ac.x1, coder.ac.x2
            xmid = x1 + (((x2 - x1) * ((p << 16) if p else 1)) >> 32)   # arithmetic_coder.rs:109-119
            bit = 1 if xmid >= 0x80000000 else 0
            m.update(bit)
            coder.encode(bit, p, w)
            longest = max(longest, int(w.s.rev_bits))
            byte = byte << 1 | bit
        out.append(byte)
    return bytes(out), longest
