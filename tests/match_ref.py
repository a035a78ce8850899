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


# ---- k_match_keys' walk: one wavefront, several blocks, the same two tagged tables (csrc/w3_match.h) ------------------------------------
TAGS = 255
WALK_MUTANTS = ["no_tag_check", "no_rezero_at_wrap", "rezero_short_table_only", "tag_mod_256", "tag_always_one_no_rezero", "pos_16_bits"]
WRAP_MUTANTS = ("no_rezero_at_wrap", "rezero_short_table_only")
WALK_STATES = ["stale_tag_rejected", "stale_pos_at_or_past_boundary", "stale_pos_past_short_last_block", "entry_cleared_at_wrap_would_have_hit",
               "long_table_only_stale", "cand_65536_or_more_back", "cand_pos_65536_or_more"]


def _walk_len(x, i, c):
    """match_len for a candidate that may lie anywhere (a stale entry taken for a live one): a byte outside the block is unequal"""
    if c == 0:
        return 0
    n, r, limit = len(x), 0, min(CAP, c)
    while r < limit and 0 <= i - 1 - r and c - 1 - r < n and x[i - 1 - r] == x[c - 1 - r]:
        r += 1
    return r


def wave_walk(data, block_size, waves, m, L, mutant=None, states=None):
    """-> the keys (8 per byte) of every block, as `waves` wavefronts leave them: wavefront w takes blocks w, w + waves, ... in turn over
    its two tables, in rounds of 64 boundaries (every lane reads the tables' state before the round, a lane's candidate is the nearest
    lower lane of the round with its hash, else the entry read; the highest lane of a group stores), entries tagged with the wavefront's
    block sequence, both tables zeroed when the tag returns to 1.  Without a mutant this equals keys() of each block alone."""
    assert mutant is None or mutant in WALK_MUTANTS
    blocks = [bytes(data[o:o + block_size]) for o in range(0, len(data), block_size)]
    out = [None] * len(blocks)
    for w in range(min(waves, len(blocks))):
        T = ({}, {})
        for seq, b in enumerate(range(w, len(blocks), waves)):
            x = blocks[b]
            n = len(x)
            short_last = b == len(blocks) - 1 and n < block_size
            if mutant == "tag_always_one_no_rezero":
                tag = 1
            else:
                tag = seq % (256 if mutant == "tag_mod_256" else TAGS) + 1
            cleared = ({}, {})
            if tag == 1 and (seq == 0 or mutant not in ("no_rezero_at_wrap", "tag_always_one_no_rezero")):
                if seq:
                    cleared = (dict(T[0]), dict(T[1]))
                T[0].clear()
                if seq == 0 or mutant != "rezero_short_table_only":
                    T[1].clear()
            c = [[0] * n, [0] * n]
            v = [[0] * n, [0] * n]
            for base in range(0, n, 64):
                hi = min(n, base + 64)
                for t, k in enumerate((m, 2 * m)):
                    seen = {}   # hash -> the highest lane of the round so far
                    for i in range(max(base, k), hi):
                        h = ctx_hash(x, i, k, L)
                        if h in seen:
                            c[t][i] = seen[h]
                        else:
                            old = T[t].get(h, 0)
                            live = old >> 24 == tag or mutant == "no_tag_check"
                            c[t][i] = (old & (0xFFFF if mutant == "pos_16_bits" else 0xFFFFFF)) if live else 0
                            if states is not None:
                                if old and not live:
                                    pos = old & 0xFFFFFF
                                    states["stale_tag_rejected"] += 1
                                    states["stale_pos_at_or_past_boundary"] += pos >= i
                                    states["stale_pos_past_short_last_block"] += short_last and pos > n
                                if not old and cleared[t].get(h, 0) >> 24 == tag:
                                    states["entry_cleared_at_wrap_would_have_hit"] += 1
                                    states["long_table_only_stale"] += t == 1
                        seen[h] = i
                        v[t][i] = _walk_len(x, i, c[t][i])
                        if states is not None and c[t][i]:
                            states["cand_65536_or_more_back"] += i - c[t][i] >= 65536
                            states["cand_pos_65536_or_more"] += c[t][i] >= 65536
                    for h, i in seen.items():   # the round's stores, after every load of the round
                        T[t][h] = ((tag << 24) | i) & 0xFFFFFFFF
            ks = []
            for i, byte in enumerate(x):
                t = 1 if v[1][i] > v[0][i] else 0
                vv, cc = v[t][i], c[t][i]
                e = x[cc] if vv and cc < n else 0
                lq = lq_of(vv) if vv else 0
                for j in range(8):
                    ks.append((lq << 1) | ((e >> (7 - j)) & 1) if vv and byte >> (8 - j) == e >> (8 - j) else 0)
            out[b] = ks
    return out


def stream_of_keys(block, ks):
    """leaf_stream from given keys"""
    x = bytes(block)
    tbl, out = {}, []
    for t, k in enumerate(ks):
        ctx = 0 if t == 0 else (k << 3) | (t & 7)
        c = tbl.get(ctx)
        if c is None:
            c = tbl[ctx] = Counter()
        out.append(c.p())
        c.update((x[t >> 3] >> (7 - (t & 7))) & 1)
    return out


def _phrase(block_size, m, seed):
    """block_size bytes without structure, but for one stretch of 2m + 1 bytes met twice: both contexts of the boundary behind the
    second occurrence hash as at the first, so an entry left by an equal block lies PAST the first boundary that looks it up (and past
    a short last block's end); in blocks of more than 64 bytes the second occurrence is in the second round"""
    p = bytearray(_lcg(block_size, 256, seed))
    r = block_size // 2 if block_size <= 64 else 64
    k = min(2 * m + 1, block_size - r)
    p[r:r + k] = p[:k]
    return bytes(p)


def _hash_sets(p, m, L):
    return tuple({ctx_hash(p, i, k, L) for i in range(k, len(p))} for k in (m, 2 * m))


def tag_phrases(block_size, m, L):
    """(A, B, C): A as _phrase says; B and C the first such phrases (by seed) whose context hashes are disjoint from A's, in both tables"""
    A = _phrase(block_size, m, 1)
    ha = _hash_sets(A, m, L)
    others, seed = [], 2
    while len(others) < 2:
        p = _phrase(block_size, m, seed)
        hp = _hash_sets(p, m, L)
        if not (ha[0] & hp[0]) and not (ha[1] & hp[1]):
            others.append(p)
        seed += 1
        assert seed < 100000, "no phrase disjoint from A"
    return A, others[0], others[1]


def tag_blocks(nblocks, block_size, waves, tail=0, m=2, L=12):
    """the steered input of the tag bookkeeping: nblocks blocks for `waves` wavefronts (block b is number b // waves of wavefront b % waves)
    plus `tail` bytes of one more.  A wavefront's blocks number 0, 255, 510, ... — where the tag is 1 again — are phrase A; all others
    alternate between B and C, which never touch A's table entries (tag_phrases).  So A's entries of block 0 are still in the tables, under
    tag 1, when block 255 comes: only the re-zeroing keeps them from passing for candidates.  Equal naive blocks cannot show that: each
    block overwrites what the one before left."""
    A, B, C = tag_phrases(block_size, m, L)
    out = bytearray()
    for b in range(nblocks + (1 if tail else 0)):
        seq = b // waves
        p = A if seq % TAGS == 0 else B if seq & 1 else C
        out += p if b < nblocks else p[:tail]
    return bytes(out)


# the shapes the GPU test runs (tests/test_gpu_match_tags.py) and tests/test_match_tags_cpu.py proves sufficient: blocks, block size, the
# wavefronts the grid is capped to, bytes of a ragged last block, (m, L)
TAG_CASES = {
    "520x24_tail_w1_2_12": (520, 24, 1, 12, 2, 12),
    "1030x12_w2_2_12": (1030, 12, 2, 0, 2, 12),
    "775x16_w3_3_12": (775, 16, 3, 0, 3, 12),
    "300x40_w1_4_16": (300, 40, 1, 0, 4, 16),
    "520x24_w1_2_8": (520, 24, 1, 0, 2, 8),      # 256 slots: B and C collide with each other (never with A)
    "520x72_w1_2_12": (520, 72, 1, 0, 2, 12),    # two rounds per block: a tag that overflows its 8 bits loses the first round's entries
}


def tag_case(name):
    nb, bs, waves, tail, m, L = TAG_CASES[name]
    return tag_blocks(nb, bs, waves, tail, m, L)


def two_block_waves(nblocks=70, block_size=24, m=2):
    """equal blocks: with 64 wavefronts, the first nblocks - 64 of them take a second block over the entries of their first"""
    return _phrase(block_size, m, 5) * nblocks


def long_block(n=70000, phrase_at=(100, 66000, 68500), seed=7):
    """one block of n bytes: filler, and a 40-byte phrase near the start, again past offset 65,536 (its candidates lie 65,536 or more
    back) and once more behind that (its candidates' POSITIONS are 65,536 or more: bits 16 .. 23 of an entry's position field)"""
    x = bytearray(_lcg(n, 256, seed))
    ph = _lcg(40, 256, seed + 1)
    for o in phrase_at:
        x[o:o + 40] = ph
    return bytes(x)
