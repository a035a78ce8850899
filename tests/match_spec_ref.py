"""The match-model leaf as a ROW OF SIXTEEN LANES decodes it (k_decode_spec<.., MATCH>: weath3rb0i_amd/csrc/w3_decode_spec.h and
w3_match_spec_plan.h), restated in plain Python on top of tests/match_ref.py — the schedule, not the definition:

  per nibble   the 15 nodes (k, x) of the nibble's tree form their contexts from the row's (e, lq) and the byte's known bits, and read
               their Counters as they stand when the nibble starts (several nodes may read one Counter: every node whose x disagrees
               with e's prefix has key 0); the data picks the path; the four path nodes update afterwards;
  per byte     after the first nibble lane r hashes the candidate word (history << 4) | r and reads T_m[h], T_2m[h]; after the second
               nibble the row takes the entries of the lane whose r is the decoded low nibble, that lane alone stores i + 1, lane 0
               stores the byte, and — once those stores have landed — ten lanes load the candidate side of the compare and e = x[c].

row_leaf_stream() must equal match_ref.leaf_stream(); each MUTANT is wrong in one behaviour.  GPU_LEAF_CASES are the single-leaf cases
tests/test_gpu_match_decode_spec.py runs, with the mutants each is meant to catch (tests/test_match_spec_walk_cpu.py proves it does)."""
from tests import match_ref as mt

MUTANTS = ["key_whole_partial", "key0_private", "cand_before_store", "store_every_lane", "e_before_store", "bound_block_len", "select_high_nibble"]
NOT_DECODED = 0xA5   # what a load of a byte that has not landed yet returns in this restatement (the output buffer's old content)


def _hash(W, k, L):
    v = W & ((1 << (8 * k)) - 1) if k < 8 else W
    return ((v * mt.MUL) & ((1 << 64) - 1)) >> (64 - L)


def _equal_bytes(a, b):
    d = a ^ b
    return 8 if d == 0 else ((d & -d).bit_length() - 1) >> 3


def _key(lq, e, part, j):
    if lq == 0 or part != e >> (8 - j):
        return 0
    return (lq << 1) | ((e >> (7 - j)) & 1)


class Row:
    """one block's row: the Counter table, the two candidate tables, (e, lq), the four rolling words of the compare's boundary side"""

    def __init__(self, m, L, n, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.m, self.L, self.n, self.mu = m, L, n, mutant
        self.ctr = {}
        self.T = [{}, {}]
        self.T_before = [{}, {}]   # the tables before the most recent boundary's store (cand_before_store reads these)
        self.e = self.lq = 0
        self.near = [0, 0, 0, 0]
        self.x = bytearray()       # the bytes that have LANDED
        self.hist = 0              # the bit history, 64 bits
        self.loads = []            # (byte index, known) of every load of decoded bytes

    def _counter(self, key):
        c = self.ctr.get(key)
        if c is None:
            c = self.ctr[key] = mt.Counter()
        return c

    def nibble(self, t, nib):
        """decode one nibble whose four bits are `nib` (MSB first), starting at step t -> the four path probabilities"""
        j0 = t & 7
        part0 = self.hist & ((1 << j0) - 1)
        nodes = {}
        for k in range(4):
            for xx in range(1 << k):
                j = j0 + k
                part = (part0 << k) | xx
                if t + k == 0:
                    ckey = 0
                else:
                    if self.mu == "key_whole_partial":   # the row-uniform known bits alone decide whether the key lives
                        key = 0 if self.lq == 0 or part0 != self.e >> (8 - j0) else (self.lq << 1) | ((self.e >> (7 - j)) & 1)
                    else:
                        key = _key(self.lq, self.e, part, j)
                    ckey = (key << 3) | j
                    if self.mu == "key0_private" and key == 0 and xx:
                        ckey = ("private", j, xx)
                nodes[(k, xx)] = self._counter(ckey)
        ps = {kx: c.p() for kx, c in nodes.items()}   # everything is read when the nibble starts
        out, xx = [], 0
        path = []
        for k in range(4):
            bit = (nib >> (3 - k)) & 1
            out.append(ps[(k, xx)])
            path.append((nodes[(k, xx)], bit))
            xx = (xx << 1) | bit
        for c, bit in path:   # four different j: four different Counters
            c.update(bit)
        self.hist = ((self.hist << 4) | nib) & ((1 << 64) - 1)
        return out

    def candidates(self, i1):
        """after the first nibble: the sixteen lanes' table reads for boundary i1"""
        T = self.T_before if self.mu == "cand_before_store" else self.T
        out = []
        for r in range(16):
            W = ((self.hist << 4) | r) & ((1 << 64) - 1)
            out.append([T[t].get(_hash(W, self.m << t, self.L), 0) if i1 >= self.m << t else 0 for t in range(2)])
        return out

    def _load(self, p, known, fresh):
        self.loads.append((p, known))
        if p == known - 1 and not fresh:
            return NOT_DECODED
        return self.x[p]

    def boundary(self, i1, byte, cand):
        """after the second nibble of byte i1 - 1 = `byte`: select, store, load, choose"""
        sel = byte >> 4 if self.mu == "select_high_nibble" else byte & 15
        c = cand[sel]
        self.T_before = [dict(self.T[0]), dict(self.T[1])]
        for r in range(16):
            if r == sel or self.mu == "store_every_lane":
                W = (self.hist & ~15) | r   # lane r's candidate word: the boundary's own word where r is the decoded low nibble
                for t in range(2):
                    if i1 >= self.m << t:
                        self.T[t][_hash(W, self.m << t, self.L)] = i1
        self.x.append(byte)   # lane 0's store; the loads below are issued after it has landed
        known = i1
        self.near = [self.hist, (self.near[1] << 8 | self.near[0] >> 56) & ((1 << 64) - 1), (self.near[2] << 8 | self.near[1] >> 56) & ((1 << 64) - 1),
                     (self.near[3] << 8 | self.near[2] >> 56) & ((1 << 64) - 1)]
        v, e = [0, 0], [0, 0]
        for t in range(2):
            ct = c[t]
            if ct == 0:
                continue
            limit = min(mt.CAP, self.n if self.mu == "bound_block_len" else ct)
            rr, q = 0, 0
            while q < limit:
                end = ct - q
                far = 0
                for s in range(8):   # one byte per load, every index inside [0, ct)
                    if s < end:
                        far |= self._load(end - 1 - s, known, True) << (8 * s)
                eq = _equal_bytes(self.near[q >> 3], far)
                rr = q + eq
                if eq < 8:
                    break
                q += 8
            v[t] = min(rr, limit)
            e[t] = self._load(ct, known, self.mu != "e_before_store")
        t = 1 if v[1] > v[0] else 0
        self.lq = mt.lq_of(v[t]) if v[t] else 0
        self.e = e[t] if v[t] else 0


def row_leaf_stream(block, m, L, mutant=None, loads=None):
    """the leaf's probabilities of one block as the row computes them"""
    x = bytes(block)
    row = Row(m, L, len(x), mutant)
    out = []
    for i, byte in enumerate(x):
        out += row.nibble(8 * i, byte >> 4)
        more = i + 1 < len(x)
        cand = row.candidates(i + 1) if more else None
        out += row.nibble(8 * i + 4, byte & 15)
        if more:
            row.boundary(i + 1, byte, cand)
    if loads is not None:
        loads += row.loads
    return out


def caught_by(block, m, L, mutants=MUTANTS):
    """the mutants (of those given) that change the leaf stream of this block"""
    want = row_leaf_stream(block, m, L)
    return {mu for mu in mutants if row_leaf_stream(block, m, L, mu) != want}


# ---- the single-leaf cases of the GPU test: name -> (input, (m, L), mutants the case is meant to catch) ---------------------------------
def _cases():
    out = {}
    meant = {
        "zeros": {"cand_before_store", "e_before_store", "bound_block_len"},   # the candidate is the byte just stored; compares stopped by the block start
        "ones_short": {"cand_before_store", "e_before_store"},                     # the same with 0xff: the block start ends the compare (zeros there)
        "period_7": {"key0_private"},                 # the candidate 7 back: what the row stored a few bytes ago; expected bytes of every shape
        "period_64": {"key0_private"},
        "mismatch_bits": {"key_whole_partial", "key0_private"},      # the key dies at each of the 8 bit positions, in either nibble
        "phrases": {"select_high_nibble"},
        "nibbles": {"select_high_nibble", "store_every_lane"},
        "pairs": {"store_every_lane"},
        "bytes": {"key0_private"},
    }
    for nm in sorted(mt.DIRECTED):
        for m, L in mt.CONFIGS:
            out["%s_%d_%d" % (nm, m, L)] = (mt.DIRECTED[nm], (m, L), meant[nm])
    out["bytes_4_20"] = (mt.DIRECTED["bytes"], (4, 20), {"key0_private"})
    return out


GPU_LEAF_CASES = _cases()
