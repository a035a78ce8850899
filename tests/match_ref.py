"""CPU truth of the match-model leaf (W3_HIST_MATCH: include/w3hip.h) for the tests, in plain Python integers — a
restatement, not the reference (which has no such history).  The leaf is OrderNEntropy(11, 3, MatchHistory(m, L)): `keys` below is
MatchHistory::hash() at every step, `Counter` is models/counter.rs:13-25, and the leaf's context is (hash << 3) | j with the block's
first step at context 0, as OrderNEntropy::update forms it.  Composed with tests/mixer_ref.py (the mixer, the oracle's coder, the
bit-by-bit model a decoder runs) and tests/apm_census.stage for whole models.

For a block x[0..n), byte boundary i, k in (m, 2m), i >= k (CAP = 32):
    v      = big-endian integer of x[i-k .. i-1];   h_k(i) = ((v * 0x9E3779B97F4A7C15) mod 2^64) >> (64 - L)
    c_k    = T_k[h_k(i)], then T_k[h_k(i)] = i      (two tables, empty = 0 at the block start)
    v_k    = 0 if c_k = 0, else the largest r <= min(CAP, c_k) with x[i-s] == x[c_k-s] for s = 1..r
    (c, v) = (c_2m, v_2m) if v_2m > v_m else (c_m, v_m);  v = 0: no prediction;  e = x[c];  lq = v for v < 16 else 16 + ((v - 16) >> 2)
    hash() at bit position j = (lq << 1) | ((e >> (7-j)) & 1) if v > 0 and (x[i] >> (8-j)) == (e >> (8-j)), else 0"""
import collections

from tests import apm_census as ac
from tests import mixer_ref as mr

CAP = 32
MUL = 0x9E3779B97F4A7C15
CONFIGS = ((2, 8), (3, 12), (4, 16))

MUTANTS = ["keep_oldest", "tie_prefers_long", "no_start_clamp", "cap_31", "lq_linear", "key_after_break", "lsb_first", "short_only",
           "little_endian_ctx"]
STATES = (["no_context", "short_only_live", "empty_slot", "v_zero", "v_below_m", "cap", "stopped_by_start", "long_wins", "tie_to_short",
           "short_longer", "cand_same_round", "cand_prev_round", "cand_64_back", "round_all_equal", "full_hit", "expect_0", "expect_1"]
          + ["v_%d" % v for v in range(1, CAP + 1)] + ["mismatch_bit_%d" % j for j in range(8)])


class Counter:
    """models/counter.rs:13-25: two u16 counts; p() = round-half-up(2^16 (c1 + 1) / (c0 + c1 + 2)); a count that reaches 65535 halves both"""
    __slots__ = ("c0", "c1")

    def __init__(self):
        self.c0 = self.c1 = 0

    def p(self):
        q = ((self.c1 + 1) << 17) // (self.c0 + self.c1 + 2)
        return (q >> 1) + (q & 1)

    def update(self, bit):
        if bit:
            self.c1 += 1
        else:
            self.c0 += 1
        if (self.c1 if bit else self.c0) == 65535:
            self.c0 = (self.c0 >> 1) + (self.c0 & 1)
            self.c1 = (self.c1 >> 1) + (self.c1 & 1)


def lq_of(v, mutant=None):
    if mutant == "lq_linear":
        return min(v, 20)
    return v if v < 16 else 16 + ((v - 16) >> 2)


def ctx_hash(x, i, k, L, mutant=None):
    v = int.from_bytes(x[i - k:i], "little" if mutant == "little_endian_ctx" else "big")
    return ((v * MUL) & ((1 << 64) - 1)) >> (64 - L)


def match_len(x, i, c, mutant=None):
    if c == 0:
        return 0
    cap = 31 if mutant == "cap_31" else CAP
    limit = min(cap, i) if mutant == "no_start_clamp" else min(cap, c)
    r = 0
    while r < limit and x[i - 1 - r] == (x[c - 1 - r] if c - 1 - r >= 0 else 0):
        r += 1
    return r


class MatchHistory:
    """the History, byte by byte: boundary(x, i) when bytes x[0..i) are known, then hash(j, part) for the j known bits `part` of byte i"""

    def __init__(self, m, L, mutant=None, states=None):
        assert 2 <= m <= 4 and 8 <= L <= 20
        self.m, self.L, self.mutant, self.states = m, L, mutant, states
        self.T = ({}, {})
        self.v, self.e, self.lq = 0, 0, 0
        self.hashes = ([], [])   # h_k of every boundary (None below k): the census of rounds

    def boundary(self, x, i):
        m, L, mu, st = self.m, self.L, self.mutant, self.states
        c, v = [0, 0], [0, 0]
        for t, k in enumerate((m, 2 * m)):
            h = None
            if i >= k and not (t == 1 and mu == "short_only"):
                h = ctx_hash(x, i, k, L, mu)
                c[t] = self.T[t].get(h, 0)
                if not (mu == "keep_oldest" and c[t]):
                    self.T[t][h] = i
                v[t] = match_len(x, i, c[t], mu)
                if st is not None:
                    if c[t] == 0:
                        st["empty_slot"] += 1
                    else:
                        if v[t] == 0:
                            st["v_zero"] += 1
                        if v[t] == c[t] < CAP:
                            st["stopped_by_start"] += 1
                        if c[t] // 64 == i // 64:
                            st["cand_same_round"] += 1
                        if c[t] // 64 == i // 64 - 1:
                            st["cand_prev_round"] += 1
                        if i - c[t] == 64:
                            st["cand_64_back"] += 1
            self.hashes[t].append(h)
        long_wins = v[1] >= v[0] and v[1] > 0 if mu == "tie_prefers_long" else v[1] > v[0]
        t = 1 if long_wins else 0
        self.v = v[t]
        self.e = x[c[t]] if v[t] else 0
        self.lq = lq_of(v[t], mu) if v[t] else 0
        if st is not None:
            if i < m:
                st["no_context"] += 1
            elif i < 2 * m:
                st["short_only_live"] += 1
            if v[1] > v[0]:
                st["long_wins"] += 1
            elif v[1] == v[0] > 0:
                st["tie_to_short"] += 1
            elif c[1] and v[1] < 2 * m and v[0] > v[1]:
                st["short_longer"] += 1   # (a true 2m-byte repeat verifies at least 2m bytes: this candidate is a collision)
            if 0 < self.v < m:
                st["v_below_m"] += 1
            if self.v:
                st["v_%d" % self.v] += 1
            if self.v == CAP:
                st["cap"] += 1

    def hash(self, j, part):
        if self.v == 0:
            return 0
        e, mu = self.e, self.mutant
        if mu != "key_after_break" and part != e >> (8 - j):
            return 0
        ebit = (e >> j) & 1 if mu == "lsb_first" else (e >> (7 - j)) & 1
        if self.states is not None:
            self.states["expect_%d" % ebit] += 1
        return (self.lq << 1) | ebit

    def byte_done(self, byte):
        if self.states is not None and self.v:
            if byte == self.e:
                self.states["full_hit"] += 1
            else:
                self.states["mismatch_bit_%d" % (8 - (byte ^ self.e).bit_length())] += 1


def keys(block, m, L, mutant=None, states=None):
    """hash() of every step of one block (8 per byte)"""
    x = bytes(block)
    h = MatchHistory(m, L, mutant, states)
    out = []
    for i, byte in enumerate(x):
        h.boundary(x, i)
        for j in range(8):
            out.append(h.hash(j, byte >> (8 - j)))
        h.byte_done(byte)
    if states is not None:
        for t, k in enumerate((m, 2 * m)):
            hs = h.hashes[t]
            for r in range(0, len(x) - 63, 64):
                if hs[r] is not None and len(set(hs[r:r + 64])) == 1:
                    states["round_all_equal"] += 1
    return out


def leaf_stream(block, m, L, mutant=None):
    """the leaf's probabilities of one block: Counter table over (hash << 3) | j, the first step at context 0"""
    x = bytes(block)
    ks = keys(x, m, L, mutant)
    tbl, out = {}, []
    for t, k in enumerate(ks):
        ctx = 0 if t == 0 else (k << 3) | (t & 7)
        c = tbl.get(ctx)
        if c is None:
            c = tbl[ctx] = Counter()
        out.append(c.p())
        c.update((x[t >> 3] >> (7 - (t & 7))) & 1)
    return out


class MatchLeaf:
    """predict() / update(bit) of the leaf, fresh for one block (what a decoder runs: it knows only the bytes it has decoded)"""

    def __init__(self, m, L):
        self.h = MatchHistory(m, L)
        self.x, self.part, self.j, self.t = bytearray(), 0, 0, 0
        self.tbl = {}
        self.h.boundary(self.x, 0)

    def predict(self):
        ctx = 0 if self.t == 0 else (self.h.hash(self.j, self.part) << 3) | self.j
        self.c = self.tbl.get(ctx)
        if self.c is None:
            self.c = self.tbl[ctx] = Counter()
        return self.c.p()

    def update(self, bit):
        self.c.update(bit)
        self.part, self.j, self.t = self.part << 1 | bit, self.j + 1, self.t + 1
        if self.j == 8:
            self.x.append(self.part)
            self.part, self.j = 0, 0
            self.h.boundary(self.x, len(self.x))


# ---- whole models: mixer_ref's leaf descriptions plus ("match", m, L) -------------------------------------------------------------------
MATCH = ("match", 4, 16)
O012 = (("o0",), ("o1",), ("on", 27, 3))
O012M = O012 + (MATCH,)


def full_cm_leaves(log_cells):
    return O012 + tuple(("slot", order, log_cells) for order in (1, 2, 3, 4)) + (MATCH,)


def w3_leaf(w3, leaf):
    return w3.MatchModel(leaf[1], leaf[2]) if leaf[0] == "match" else mr.w3_leaf(w3, leaf)


def w3_model(w3, leaves, combine="mix", select=mr.ORDER0, rate=14, stages=()):
    """combine: "mix" = LogisticMixer over the leaves, "tree" = a left-leaning BestOfTwo tree, "leaf" = the single leaf"""
    ls = [w3_leaf(w3, lf) for lf in leaves]
    if combine == "mix":
        m = w3.LogisticMixer(ls, select, rate)
    else:
        m = ls[0]
        for nxt in ls[1:]:
            m = w3.BestOfTwoModel(m, nxt)
    for kind, srate in stages:
        m = w3.APM(m, kind, srate)
    return m


def leaf_streams(orc, leaves, block, mutant=None):
    return [leaf_stream(block, lf[1], lf[2], mutant) if lf[0] == "match" else mr.leaf_streams(orc, (lf,), block)[0] for lf in leaves]


def tree(streams):
    """a BestOfTwo tree of any shape: the leftmost leaf of maximal |p - 1/2| (models/mod.rs:67-69)"""
    out = []
    for ps in zip(*streams):
        best = ps[0]
        for p in ps[1:]:
            if abs(p - 32768) > abs(best - 32768):
                best = p
        out.append(best)
    return out


def predict_block(orc, leaves, block, combine="mix", select=mr.ORDER0, rate=14, stages=(), mutant=None):
    streams = leaf_streams(orc, leaves, block, mutant)
    p = mr.mix(streams, block, select, rate) if combine == "mix" else tree(streams)
    for kind, srate in stages:
        p = ac.stage(p, bytes(block), kind, srate, with_kinds=False)[0]
    return p


def predict_blocks(orc, leaves, data, block_size, combine="mix", select=mr.ORDER0, rate=14, stages=()):
    out = []
    for blk in mr.blocks_of(data, block_size):
        out += predict_block(orc, leaves, blk, combine, select, rate, stages)
    return out


def encode_blocks(orc, leaves, data, block_size, combine="mix", select=mr.ORDER0, rate=14, stages=()):
    """-> (streams: bytes, block_lens: list, block_bits: list)"""
    streams, lens, bits = [], [], []
    for blk in mr.blocks_of(data, block_size):
        s, b = mr.code_block(orc, predict_block(orc, leaves, blk, combine, select, rate, stages), blk)
        streams.append(s)
        lens.append(len(s))
        bits.append(b)
    return b"".join(streams), lens, bits


class Incremental(mr.Incremental):
    """mixer_ref's bit-by-bit model with the match leaf among its leaves (logistic mixer over them, APM stages behind)"""

    def __init__(self, orc, leaves, select=mr.ORDER0, rate=14, stages=()):
        self.leaves = [MatchLeaf(lf[1], lf[2]) if lf[0] == "match" else mr.orc_leaf(orc, lf) for lf in leaves]
        n = len(leaves)
        self.select, self.rate = select, rate
        self.w = [[65536 // n] * n for _ in range(256 if select == mr.ORDER0 else 1)]
        self.apm = [mr._Apm(k, r) for k, r in stages]
        self.c0, self.c1 = 1, 0


def decode_blocks(orc, leaves, comp, block_lens, block_size, orig_len, select=mr.ORDER0, rate=14, stages=()):
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


# ---- directed inputs (at most 4 KiB each) -----------------------------------------------------------------------------------------------
def _lcg(n, mod, seed):
    out, s = bytearray(), seed
    for _ in range(n):
        s = (s * 1103515245 + 12345) & 0x7FFFFFFF
        out.append((s >> 16) % mod)
    return bytes(out)


def _phrases():
    """a few phrases met again after other text: the 2m-byte context finds the long repeat while the m-byte context's most recent
    occurrence is a shorter one (long wins); the same phrases back to back (ties)"""
    words = [b"the quick brown fox ", b"jumps over ", b"a lazy dog; ", b"quick brown cat ", b"over a lazy fox, ", b"brown dog jumps "]
    order = _lcg(300, len(words), 99)
    return b"".join(words[k] for k in order)[:4096]


def _mismatch_at_each_bit():
    """eight distinct 8-byte contexts P_j, each followed by 0x55 and, at its second occurrence, by 0x55 with bit j (MSB first) flipped"""
    out = bytearray()
    for j in range(8):
        p = bytes(8 * j + t + 1 for t in range(8))
        out += p + b"\x55" + p + bytes([0x55 ^ (0x80 >> j)])
    return bytes(out)


DIRECTED = {
    "zeros": bytes(4096),                                  # every lane of a round equal, every length up to the cap, compares stopped by the block start
    "ones_short": b"\xff" * 70,                            # the same with expected bit 1, across one round boundary
    "period_64": bytes(range(64)) * 16,                    # the candidate exactly 64 back
    "period_7": bytes([3, 1, 4, 1, 5, 9, 2]) * 100,        # candidates inside the same round
    "phrases": _phrases(),
    "mismatch_bits": _mismatch_at_each_bit(),
    "nibbles": _lcg(4096, 16, 5),                          # collisions with a few bytes of chance agreement
    "bytes": _lcg(4096, 256, 11),                          # collisions at L = 8: candidates that verify nothing
    "pairs": _lcg(4096, 2, 3),                             # two symbols: long matches of every length, broken at random
}


def reached(name, m, L):
    st = collections.Counter()
    keys(DIRECTED[name], m, L, states=st)
    return st
