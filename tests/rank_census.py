"""A CPU model of which states of the rank kernels one block reaches, and the inputs built to reach every one of them: test
infrastructure, no device code and no oracle.  tests/test_rank_census_cpu.py asserts that the inputs reach the states;
tests/test_gpu_rank_rounds.py runs the same bytes through the kernels.

What is restated here, from weath3rb0i_amd/csrc/w3_predict.h (line numbers of that file) and w3_apm.h:

Records and groups.  A block's record of position i is (i, window c0 | c1 << 8 | c2 << 16 | c3 << 24), c_k = the byte k places before
position i, zero before the block start (load_window, w3_window.h:21-30).  The records are sorted stably by the group:
  order1           group c1 (k_partition8<1> :625, k_partition<1> :540-544);           low key byte ck = c2 (:934)
  order2_c2_major  group (c1, c2), chained behind an Order1 leaf: the records sorted by c1 are sorted stably by c2
                   (k_partition8<3> :625 / :630, k_partition<3> :535-539), so c2 is the major key;   ck = c3
  order2_c1_major  group (c1, c2) from scratch (k_partition<2> :546-553, least significant digit first);  ck = c3
Keys: key_j = ((ck << 8 | c0) >> (8 - j)) & 0xFF (:948), coded bit j = (c0 >> (7 - j)) & 1.

Splits (:557-576 serial search, :806-816 binary search over the bin ends, :817-855 eight at a time): sp[0] = 0, sp[64] = len, sp[s] = the
first group head at an index >= s * len // 64, or len.  Of the eight-at-a-time search: a boundary whose 64 records from the ideal point
hold no head (:838-841) takes the boundary before it when that one is not below its own ideal point (`before`, :844), else walks on
64 records at a time (:845-850).

k_rank_sorted (:888-1023), per non-empty slice (job): the table is cleared (:904), exact = false (unless the context runs without LDS
atomics), dirty = false, open_g = none.  Rounds of 64 records from the slice start; heads = lanes whose group differs from the lane
before, lane 0 compared with open_g and counted whatever it is (:940); the round takes the LDS-add path iff !exact and heads <=
maxseg = 4 (:954).  `dirty` is true from the slice's second round on (:1013), open_g = the group of the round's last valid lane (:1014),
so a round's lane 0 is NEW iff it is the slice's first round or its group differs from the record before it; CARRIED otherwise.
Whole-table clears: the slice start (:904); LDS-add round, dirty and lane 0 new (:962-966); LDS-add round, the carried group ends inside
the round (:977-979); ballot round, dirty and the last lane's group is not open_g (:999-1003).  The latch: exact = some returned packed
count >= 65400 (:993, :230, :245-250), for the rest of the slice.  A returned count is the number of earlier records of the same group
with the same key_j and coded bit 0 (low half) or 1 (high half): the table is the exact Counter state of the open group on either
path, and nothing halves below 65535.  Records are staged in batches of PF rounds (:914-922), PF = 8, or 4 in the eight-wavefront
instance (w3_twophase.h:574-579).

k_apm1 (w3_apm.h:359-459), over the same slices of the order1 records: rounds of 8 records; open_g = none at the slice start, then the
group of the record before the round.  A round all of whose valid records are in open_g takes the fast path (:423-428); any other is
committed record by record, with a table initialisation wherever the group changes (:439-448)."""
import collections

import numpy as np

FORMS = ("order1", "order2_c2_major", "order2_c1_major")
SLICES = 64
MAXSEG = 4
LIM = 65400
PFS = (8, 4)

ROUND_STATES = ["add.seg4", "ballot.seg5", "add.carried_ends", "ballot.carried_ends", "add.carried_fills", "add.new_at_lane0",
                "ballot.new_at_lane0", "switch.add_to_ballot", "switch.ballot_to_add", "add.partial_last", "ballot.partial_last"]
BATCH_STATES = ["pf%d.%s" % (pf, s) for pf in PFS for s in ("head_on_batch", "group_across_batch")]
LATCH_STATES = ["latch", "latch.carried_ends_after", "latch.group_change_after"]
SLICE_STATES = ["slice.short", "slice.ragged", "slice.empty"] + ["pf%d.slice_over_two_batches" % pf for pf in PFS]
SPLIT_STATES = ["split.ideal_on_head", "split.walk", "split.shortcut", "split.boundary_is_len", "split.block_under_64"]
APM1_STATES = ["apm1.fast", "apm1.boundary_inside", "apm1.first_opens_group", "apm1.first_opens_group_mid_slice", "apm1.partial_last"]
RANK_STATES = ROUND_STATES + BATCH_STATES + LATCH_STATES + SLICE_STATES + SPLIT_STATES


def records(block, form):
    """-> (pos, g, c0, ck) of the block's records in sorted order"""
    b = np.frombuffer(bytes(block), dtype=np.uint8).astype(np.uint32)
    n = len(b)
    c = [b] + [np.concatenate([np.zeros(min(k, n), dtype=np.uint32), b[:max(n - k, 0)]]) for k in (1, 2, 3)]
    if form == "order1":
        g, sort_key, ck = c[1], c[1], c[2]
    else:
        g, ck = c[1] | (c[2] << 8), c[3]
        sort_key = (c[2] << 8 | c[1]) if form == "order2_c2_major" else (c[1] << 8 | c[2])
    pos = np.argsort(sort_key, kind="stable")
    return pos, g[pos], c[0][pos], ck[pos]


def head_flags(g):
    h = np.ones(len(g), dtype=bool)
    h[1:] = g[1:] != g[:-1]
    return h


def splits(g):
    """sp[0 .. 64] of the sorted groups g"""
    n = len(g)
    heads = np.flatnonzero(head_flags(g))
    sp = [0]
    for s in range(1, SLICES):
        k = int(np.searchsorted(heads, s * n // SLICES, "left"))
        sp.append(int(heads[k]) if k < len(heads) else n)
    return sp + [n]


def split_states(g, sp, st):
    n = len(g)
    h = head_flags(g)
    if n < 64:
        st["split.block_under_64"] += 1
    for s in range(1, SLICES):
        ideal = s * n // SLICES
        if sp[s] == n:
            st["split.boundary_is_len"] += 1
        if 0 < ideal < n and h[ideal]:
            st["split.ideal_on_head"] += 1
        if not h[ideal:min(ideal + 64, n)].any():       # (:838: no head among the 64 records from the ideal point)
            if s > 1 and sp[s - 1] >= ideal:
                st["split.shortcut"] += 1
            else:
                st["split.walk"] += 1


def _hot(g, c0, ck, lo, hi):
    """per record of the slice [lo, hi): an LDS-add round would return a count >= LIM for it.  Only groups of LIM records or more can."""
    hot = np.zeros(hi - lo, dtype=bool)
    starts = np.flatnonzero(head_flags(g[lo:hi]))
    ends = np.append(starts[1:], hi - lo)
    for a, e in zip(starts, ends):
        if e - a < LIM:
            continue
        w16 = (ck[lo + a:lo + e] << 8) | c0[lo + a:lo + e]
        byte = c0[lo + a:lo + e]
        for j in range(8):
            key = (w16 >> (8 - j)) & 0xFF
            bit = (byte >> (7 - j)) & 1
            order = np.argsort(key, kind="stable")
            ks, bs = key[order], bit[order].astype(np.int64)
            run_start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
            run_id = np.cumsum(np.r_[True, ks[1:] != ks[:-1]]) - 1
            for ind in (1 - bs, bs):
                excl = np.cumsum(ind) - ind
                excl -= excl[run_start][run_id]
                h = np.zeros(e - a, dtype=bool)
                h[order] = excl >= LIM
                hot[a:e] |= h
    return hot


def rank_states(g, c0, ck, sp, st, no_latch=False):
    """k_rank_sorted's rounds over the slices sp of one block's sorted records"""
    for s in range(SLICES):
        lo, hi = sp[s], sp[s + 1]
        n = hi - lo
        if n <= 0:
            st["slice.empty"] += 1
            continue
        if n < 64:
            st["slice.short"] += 1
        if n % 64:
            st["slice.ragged"] += 1
        h = head_flags(g[lo:hi])
        for pf in PFS:
            if n > 2 * pf * 64:
                st["pf%d.slice_over_two_batches" % pf] += 1
            edges = np.arange(pf * 64, n, pf * 64)
            st["pf%d.head_on_batch" % pf] += int(h[edges].sum())
            st["pf%d.group_across_batch" % pf] += int((~h[edges]).sum())
        bases = np.arange(0, n, 64)
        inner = h.copy()
        inner[bases] = False
        nseg = 1 + np.add.reduceat(inner.astype(np.int64), bases)
        lane0_new = h[bases]
        hot = None
        if not no_latch and (np.diff(np.append(np.flatnonzero(h), n)) >= LIM).any():
            hot = np.add.reduceat(_hot(g, c0, ck, lo, hi).astype(np.int64), bases) > 0
        exact, prev_add = False, None
        for r in range(len(bases)):
            k, new0, valid = int(nseg[r]), bool(lane0_new[r]), min(64, n - 64 * r)
            add = not exact and k <= MAXSEG
            p = "add." if add else "ballot."
            carried = r > 0 and not new0
            if exact:
                if carried and k > 1:
                    st["latch.carried_ends_after"] += 1
                if k > 1 or new0:
                    st["latch.group_change_after"] += 1
            else:
                if k == 4:
                    st["add.seg4"] += 1
                if k == 5:
                    st["ballot.seg5"] += 1
                if carried and k > 1:
                    st[p + "carried_ends"] += 1
                if carried and k == 1 and valid == 64:
                    st["add.carried_fills"] += 1
                if r > 0 and new0:
                    st[p + "new_at_lane0"] += 1
                if carried and prev_add is not None and prev_add != add:
                    st["switch.add_to_ballot" if prev_add else "switch.ballot_to_add"] += 1
                if valid < 64:
                    st[p + "partial_last"] += 1
            if add and hot is not None and hot[r]:
                exact = True
                st["latch"] += 1
            prev_add = add


def apm1_states(g, sp, st):
    """k_apm1's rounds of 8 over the slices of the order1 records"""
    for s in range(SLICES):
        lo, hi = sp[s], sp[s + 1]
        n = hi - lo
        if n <= 0:
            continue
        h = head_flags(g[lo:hi])
        bases = np.arange(0, n, 8)
        inner = h.copy()
        inner[bases] = False
        inside = np.add.reduceat(inner.astype(np.int64), bases) > 0
        first = h[bases]
        st["apm1.fast"] += int((~inside & ~first).sum())
        st["apm1.boundary_inside"] += int(inside.sum())
        st["apm1.first_opens_group"] += int(first.sum())
        st["apm1.first_opens_group_mid_slice"] += int(first[1:].sum())
        if n % 8:
            st["apm1.partial_last"] += 1


def census(block, form):
    """-> (Counter of the states one block reaches as a leaf of `form`, with k_apm1's for order1; its split table)"""
    st = collections.Counter()
    pos, g, c0, ck = records(block, form)
    sp = splits(g)
    split_states(g, sp, st)
    rank_states(g, c0, ck, sp, st)
    if form == "order1":
        apm1_states(g, sp, st)
    return +st, sp


def describe(block, form, position):
    """where the record of `position` falls for a leaf of `form`: its slice, round and lane, and what the model says of that round"""
    pos, g, c0, ck = records(block, form)
    sp = splits(g)
    idx = int(np.flatnonzero(pos == position)[0])
    s = max(k for k in range(SLICES) if sp[k] <= idx < sp[k + 1])
    lo, hi = sp[s], sp[s + 1]
    r, lane = divmod(idx - lo, 64)
    h = head_flags(g[lo:hi])
    rnd = h[64 * r:64 * r + 64]
    k = 1 + int(rnd[1:].sum())
    return ("%s: sorted index %d, slice %d [%d, %d), round %d lane %d, group 0x%x; the round has %d group(s) (%s unless latched), lane 0 %s, %d valid lanes"
            % (form, idx, s, lo, hi, r, lane, int(g[idx]), k, "LDS-add path" if k <= MAXSEG else "ballot path",
               "opens a group" if rnd[0] else "carries the group on", len(rnd)))


def census_blocks(data, block_size, form):
    """the states of every block of `data` together"""
    st = collections.Counter()
    for o in range(0, len(data), block_size):
        st += census(data[o:o + block_size], form)[0]
    return st


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
GROUP_SIZES = (1, 2, 3, 5, 13, 16, 60, 64, 100, 128, 448, 512, 576, 1100)


def histogram_block(seed, nvals, order, chunk=0):
    """a byte histogram with counts drawn from GROUP_SIZES (an Order1 group per byte value, as long as its count), laid out sorted
    (order-2 groups as long as the Order1 groups), shuffled (short order-2 groups), or in shuffled chunks of up to `chunk` equal bytes"""
    rng = np.random.default_rng(seed)
    vals = rng.permutation(256)[:nvals].astype(np.uint8)
    b = np.repeat(vals, rng.choice(GROUP_SIZES, nvals))
    if order == "sorted":
        b = np.sort(b)
    elif order == "shuffled":
        rng.shuffle(b)
    else:
        b = np.sort(b)
        cuts = np.flatnonzero(rng.random(len(b) - 1) < 2.0 / chunk) + 1
        parts = np.split(b, cuts)
        b = np.concatenate([parts[k] for k in rng.permutation(len(parts))])
    return b.tobytes()


def clustered_block(seed):
    """a dozen long Order1 groups and, between them, 192 neighbouring byte values of 1 .. 13 records each: slices of two and three
    rounds with more than four Order1 groups per round (an Order1 leaf has at most 256 groups, so most inputs give it none)"""
    rng = np.random.default_rng(seed)
    counts = np.zeros(256, dtype=np.int64)
    counts[32:224] = rng.choice((1, 2, 3, 5, 8, 13), 192)
    big = np.r_[rng.permutation(32)[:6], 224 + rng.permutation(32)[:6]]
    counts[big] = rng.choice((100, 128, 448, 512, 576, 1100), 12)
    counts[[64, 96, 128, 160, 192]] = (60, 64, 100, 64, 60)      # (groups of a round or so inside the cluster: path switches with a group carried across)
    b = np.repeat(np.arange(256, dtype=np.uint8), counts)
    rng.shuffle(b)
    return b.tobytes()


def batch_head_block(pf):
    """pf * 64 - 1 zero bytes, then random non-zero bytes: the all-zero group is exactly one staging batch of the block's first slice"""
    rng = np.random.default_rng(pf)
    n = 40000 if pf == 8 else 20000
    z = pf * 64 - 1
    return bytes(z) + rng.integers(1, 256, n - z, dtype=np.uint8).tobytes()


def latch_block():
    """66,000 x 'e' (a group whose counts pass 65400 and then 65535) and a tail of short and long groups"""
    rng = np.random.default_rng(66)
    tail = np.repeat(np.arange(0x66, 0x66 + 20, dtype=np.uint8), 200)
    rng.shuffle(tail)
    return b"e" * 66000 + tail.tobytes()


def heads_on_ideal_block():
    """64 Order1 groups of 100 records in a block of 6,400 (group 0 is the block's first record and the 99 that follow a zero byte; the
    block's last byte has no successor): every ideal point of the split search is a group head, in every leaf form"""
    return np.repeat(np.arange(64, dtype=np.uint8), [99] + [100] * 62 + [101]).tobytes()


def long_last_group_block():
    """short groups, then one group of more than half the block: ideal points inside it with no head within 64 records, boundaries
    equal to the block's length"""
    rng = np.random.default_rng(9)
    head = np.repeat(np.arange(1, 41, dtype=np.uint8), rng.integers(1, 90, 40))
    return head.tobytes() + b"\xf0" * 5000


def tiny_block():
    """fewer than 64 records"""
    return b"abracadabra, abracadabra: 37 records."


def after_latch_block():
    """5,000,000 bytes in sorted runs: 0x20 x 234,374 (its group, behind the one record of group 0, ends where the third ideal point
    78,125 * 3 falls), 'e' x 66,000 (opens slice 3 and latches it), the rest spread evenly over 0x66 .. 0xff: slice 3 goes on with
    further groups after the latch.  Only a block of more than 64 * 65400 records can do that: in a smaller one an ideal point
    falls inside the latching group and ends the slice there."""
    n, a, e = 5_000_000, 234_374, 66_000
    vals = np.arange(0x66, 0x100)
    rest = n - a - e
    counts = np.full(len(vals), rest // len(vals))
    counts[:rest % len(vals)] += 1
    return b"\x20" * a + b"e" * e + np.repeat(vals.astype(np.uint8), counts).tobytes()


SMALL_INPUTS = {
    "hist_sorted": lambda: histogram_block(1, 30, "sorted"),
    "hist_shuffled": lambda: histogram_block(2, 24, "shuffled"),
    "hist_chunk40": lambda: histogram_block(3, 28, "chunks", 40),
    "hist_chunk150": lambda: histogram_block(4, 40, "chunks", 150),
    "hist_chunk12": lambda: histogram_block(5, 20, "chunks", 12),
    "clustered_a": lambda: clustered_block(18),
    "clustered_b": lambda: clustered_block(7),
    "batch_head_pf8": lambda: batch_head_block(8),
    "batch_head_pf4": lambda: batch_head_block(4),
    "latch": latch_block,
    "heads_on_ideal": heads_on_ideal_block,
    "long_last_group": long_last_group_block,
    "tiny": tiny_block,
}
LARGE_INPUT = "after_latch"
_cache = {}


def block(name):
    """the named input, made once"""
    if name not in _cache:
        _cache[name] = after_latch_block() if name == LARGE_INPUT else SMALL_INPUTS[name]()
    return _cache[name]


def block_census(name, form):
    if (name, form) not in _cache:
        _cache[(name, form)] = census(block(name), form)
    return _cache[(name, form)]
