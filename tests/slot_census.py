"""A CPU model of which Cell states, pipeline cases and replay cases of the slot-state leaf one block reaches, and the inputs built
to reach every one of them: test infrastructure, no device code.  tests/test_slot_census_cpu.py checks the model against the oracle
step for step and asserts that the inputs reach the kinds; tests/test_gpu_slot_cells.py runs the same bytes through the kernels.

What is restated here (line numbers of oracle/w3_oracle.c unless a file is named):

The state table (st_build :879-902 over st_next_nodes :864-877 and st_calc_prob :859-862): a lattice of 44 levels, level L holding L
nodes, in four copies a, b, c, d behind the three entry states 0, 1, 2; a step with bit 0 / 1 from copy a or c goes to copy a / b,
from copy b or d to copy c / d.  Level 44 steps back to level 22, except that its end nodes keep themselves on a 0 (node 0) or a 1
(node 43): states 949 (copy a) and 3962 (copy d) loop on themselves.  The confidence of a state (conf_build :986-994) is 0 for the
root, 1 for the states 1 and 2, level + 1 inside a copy: at most 45.

The hash (w3o_slot_hash :998-1006): splitmix64's finaliser over k = (the last `order` bytes, most recent lowest) << 8 | marker, marker 0
for a byte's first nibble and 0x10 | first nibble for its second, plus (order + 1) * 0x9E3779B97F4A7C15.  The bytes before the block
are zero (slot_reset :1045-1049).  The Cell is the hash's top log_cells bits (:926-928), the tag its low 12 (:1028).

slot_select (:1025-1043): the tag is compared with the Cell's tags in the order 3, 2, 1, 0 (:1030); an empty Cell's tags are 0, so a
context of tag 0 hits slot 3 of an empty Cell and nothing is cleared.  On a miss the victim is the slot whose first-bit state has the
least confidence, candidates in the order 1, 0, 2, 3 with a strict < (:1032-1037); its tag is stored and its 15 states are cleared
(:1038-1040).  slot_update (:1059-1069): the four states of a nibble are node (1 << bit_id) - 1 + (the nibble's bits so far) of the
slot; state q = 15 * slot + node of a Cell occupies the three nibbles from nibble 3 q of the Cell's 90 state bytes
(w3o_slot_get_idx :939-943, hashmap.rs:80-84), so q shares a byte with q + 1 when q is even and with q - 1 when it is odd.

The event order of a block: event e is nibble e & 1 (0 = the high one) of byte e >> 1; step 8 i + 4 h + k is bit k of nibble h of byte i.

k_slot (weath3rb0i_amd/csrc/w3_slot.h:145-219): a lane per block; the Cell of event e is in LDS, those of e + 1 and e + 2 in flight.
When e ends the lane keeps the LDS copy if c[e+1] = c[e] (:209), takes G, the Cell of e - 1 as it was written back, if c[e+1] =
c[e-1] (:209, :214), and the prefetch otherwise; G is read back only when some lane of the wavefront has c[e+2] = c[e] (:203).  The
prefetch of e + 2 is issued when e starts (:185), so a Cell that e - 1 wrote comes back to e + 2 through memory.  Lanes past the last
block mirror it with length 0 (:115-119).  This model counts those cases over the events that exist; a lane past its block's end
still votes in the ballot of :203, which costs a read-back and changes nothing.

k_slot_replay (w3_slot2.h:253-345, twophase_predict_b w3_twophase.h:631-642): leaf_w = min(2^log_cells, 1024) / 64 wavefronts per
(block, leaf), at least 1 and at most 4; fine bin = cell >> max(log_cells - 10, 0); lane L of the 64 leaf_w lanes owns the fine bins
[L * nbins // lanes, (L + 1) * nbins // lanes) (:286-292) and replays their records, sorted stably by Cell, in chunks of 8 (:311-341).
The sort (k_slot_sort :119-185) runs in tiles of 2,048 events and takes a second pass above 2^8 Cells (w3_twophase.h:605)."""
import collections

import numpy as np

MAX_LEVEL = 44
ST_AUX = MAX_LEVEL * (MAX_LEVEL + 1) // 2      # 990
ST_SIZE = 3 + 4 * ST_AUX                       # 3963
GOLD = 0x9E3779B97F4A7C15
PIN0, PIN1 = 949, 3962


def _state_table():
    aux_p, aux_n = [], []
    filled = 0
    for level in range(1, MAX_LEVEL + 1):
        for node in range(level):
            aux_p.append(((1 << 16) * (node + 1) // (level - 1 + 2)) & 0xFFFF)
            if level == MAX_LEVEL:
                nn = ((node + 2) // 2 - 1) + (22 - 1) * 22 // 2
                cur = filled + node
                aux_n.append((cur if node == 0 else nn, cur if node == level - 1 else nn))
            else:
                aux_n.append((filled + level + node, filled + level + node + 1))
        filled += level
    a, b, c, d = 3, 3 + ST_AUX, 3 + 2 * ST_AUX, 3 + 3 * ST_AUX
    prob, n0, n1, conf = [0] * ST_SIZE, [0] * ST_SIZE, [0] * ST_SIZE, [0] * ST_SIZE
    prob[0:3] = [1 << 15] * 3
    n0[0:3], n1[0:3] = [1, a, c], [2, b, d]
    conf[1] = conf[2] = 1
    filled = 0
    for level in range(1, MAX_LEVEL + 1):
        for node in range(level):
            i = filled + node
            for base, t0, t1 in ((a, a, b), (b, c, d), (c, a, b), (d, c, d)):
                prob[base + i], n0[base + i], n1[base + i], conf[base + i] = aux_p[i], t0 + aux_n[i][0], t1 + aux_n[i][1], level + 1
        filled += level
    return prob, n0, n1, conf


PROB, NEXT0, NEXT1, CONF = _state_table()


def mix(k):
    """splitmix64's finaliser on a uint64 array"""
    k = k ^ (k >> np.uint64(30))
    k = k * np.uint64(0xBF58476D1CE4E5B9)
    k = k ^ (k >> np.uint64(27))
    k = k * np.uint64(0x94D049BB133111EB)
    return k ^ (k >> np.uint64(31))


def context_hash(order, hist, marker):
    """hist: the last bytes, most recent lowest (uint64 array); marker: 0, or 0x10 | first nibble"""
    with np.errstate(over="ignore"):
        k = hist & np.uint64((1 << (8 * order)) - 1) if order else np.zeros_like(hist)
        k = (k << np.uint64(8)) | marker.astype(np.uint64)
        return mix(k + np.uint64(((order + 1) * GOLD) & (2**64 - 1)))


def hashes(block, order):
    """the hash of every nibble event of the block"""
    b = np.frombuffer(bytes(block), dtype=np.uint8).astype(np.uint64)
    n = len(b)
    hist = np.zeros(n, dtype=np.uint64)
    for k in range(1, min(order, 7) + 1):
        hist |= np.concatenate([np.zeros(min(k, n), dtype=np.uint64), b[:max(n - k, 0)]]) << np.uint64(8 * (k - 1))
    h = np.empty(2 * n, dtype=np.uint64)
    h[0::2] = context_hash(order, hist, np.zeros(n, dtype=np.uint64))
    h[1::2] = context_hash(order, hist, np.uint64(0x10) | (b >> np.uint64(4)))
    return h


def cells_of(block, order, log_cells):
    return (hashes(block, order) >> np.uint64(64 - log_cells)).astype(np.int64)


# ---- kinds ----------------------------------------------------------------------------------------------------------------------------
VICTIM_KINDS = ["miss.victim1.strict", "miss.victim0.strict", "miss.victim2.strict", "miss.victim3.strict",
                "miss.tie.all4_to_1", "miss.tie.0eq2_to_0", "miss.tie.2eq3_to_2", "miss.tie.1_and_one_later_to_1"]
PACKED_KINDS = ["packed.%d" % q for q in range(60)]
# miss.tie.tag0_entrant: a miss whose least confidence is shared, one of the sharers being a slot whose context came in as a tag-0 hit on
# an empty slot 3 and not as a victim.  That context sits in the slot the candidate order names last without having been ranked by it,
# which is what tells the tag compare order and the strictness of < from a renaming of the slots (EQUIVALENT_MUTANTS).
CELL_KINDS = (["hit.0", "hit.1", "hit.2", "hit.3", "falsehit", "tag0.empty_cell", "tag0.slot3_empty_others_owned", "miss.tag0", "miss.tie.tag0_entrant"]
              + VICTIM_KINDS + [k + ".conf8" for k in VICTIM_KINDS] + ["miss.tie.all4.conf20", "evict.return", "state.pinned_949", "state.pinned_3962"]
              + PACKED_KINDS)
PIPE_RELATIONS = ["next_same", "next_is_prev", "next_other", "e2_same", "e2_is_prev"]
PIPELINE_KINDS = (["pipe.%s.%s.%s" % (r, par, upd) for r in PIPE_RELATIONS for par in ("even", "odd") for upd in ("plain", "evict")]
                  + ["pipe.block_of_1", "pipe.block_of_2", "pipe.block_of_3"])
LAYOUT_KINDS = ["layout.e2_same_some_lanes", "layout.e2_same_none_then_some", "layout.unequal_lanes", "layout.mirrored_lanes"]
REPLAY_KINDS = ["replay.leaf_w1", "replay.leaf_w2", "replay.leaf_w4", "replay.fewer_bins_than_lanes", "replay.cells_share_a_bin", "replay.one_pass",
                "replay.two_passes", "replay.idle_lane_beside_busy", "replay.one_lane_has_all", "replay.count_1", "replay.count_7", "replay.count_8",
                "replay.count_9", "replay.count_16", "replay.count_below_maxc", "replay.cell_change_at_chunk_start", "replay.cell_change_mid_chunk",
                "replay.slot_first_touched_after_another", "replay.evict_then_reuse", "replay.tile_2046", "replay.tile_2048", "replay.tile_2050"]
# A tag-0 hit on an EMPTY slot of id < 3.  The tags are compared 3, 2, 1, 0, so it needs slot 3's tag to be non-zero.  Slot 3 only
# receives a non-zero tag as a victim, and 3 is the last candidate under a strict <: its confidence is then below those of 1, 0 and 2,
# which are therefore at least 1.  A first-bit state leaves 0 only when its slot's nibble is walked, and a slot walked is owned from
# then on (an eviction hands it to another context and walks it at once).  So 1, 0 and 2 are owned and no slot below 3 is empty.
UNREACHABLE = {"tag0.hit_empty_below_3": "slot 3 takes a non-zero tag only as the strict minimum of four, which needs 1, 0 and 2 owned"}

# Deliberately wrong models.  A mutant named flip:<kind> takes, at the events of that miss kind and nowhere else, the wrong victim: of the
# three other slots the one with the MOST confidence, the last candidate among equals.  (Taking the other tied slot instead would show much
# less: between two slots of equal confidence it often only swaps which of them is called what.)
FLIP_KINDS = VICTIM_KINDS + [k + ".conf8" for k in VICTIM_KINDS] + ["miss.tie.all4.conf20"]
MUTANTS = (["tag0_is_miss", "tag0_miss_no_clear", "no_clear_on_evict", "conf_cap_7", "full_hash", "no_self_loop", "le_for_lt", "tags_0_to_3"]
           + ["skip_cand_%d" % k for k in range(4)]
           + ["no_match_%d" % k for k in range(4)] + ["drop_neighbour_%d" % q for q in range(60)] + ["flip:" + k for k in FLIP_KINDS])
# Wrong on paper and right in every prediction: the candidate order 0, 1, 2, 3.  It is the true model with the names 0 and 1 of every
# Cell's slots swapped, and a prediction never depends on a slot's name.  The swap leaves the tag compare order 3, 2, {1, 0} as it is but
# for the last two, and those two are only ever told apart by a tag both could hold: the tags of a Cell's owned slots are distinct (a
# tag enters on a miss, or as the tag-0 hit on empty slot 3), and an empty slot below 3 is never hit (UNREACHABLE).  So the compare
# finds the same context, and the victim is picked by confidence and rank alone.  tests/test_slot_census_cpu.py asserts the equality
# on every input, so that nobody takes it for a mutant a test could kill.
# <= for < and the tags compared 0 .. 3 are NOT renamings, although they look like it: <= turns the candidate order round (3, 2, 0, 1 under
# <) and leaves the tag compare alone; the other turns the tag compare round and leaves the candidates alone.  A tag-0 context that hits an
# empty Cell's slot (3 in the oracle, the last candidate; 0 with the tags compared 0 .. 3, the second candidate; 3 under <=, now the first
# candidate) gets another rank against its neighbours, and a later tie at the minimum evicts another context.  Both are in MUTANTS,
# and the kind miss.tie.tag0_entrant with the input tag0_entrant_tie is there to kill them.
EQUIVALENT_MUTANTS = ["cand_order_0123"]
# the kinds (names with _ are helpers, counted but not required) at whose events a mutant may first decide differently
MUTANT_SCOPE = {"tag0_is_miss": {"_tag0.empty_slot"}, "tag0_miss_no_clear": {"miss.tag0"}, "no_clear_on_evict": {"_evict.live"},
                "conf_cap_7": {"_miss.conf_gt7"}, "full_hash": {"falsehit"}, "no_self_loop": {"state.pinned_949", "state.pinned_3962"},
                "le_for_lt": {"_miss.tie"}, "tags_0_to_3": {"_tag0.empty_slot"}}
for _k in range(4):
    MUTANT_SCOPE["skip_cand_%d" % _k] = {"_miss.victim%d" % _k}
    MUTANT_SCOPE["no_match_%d" % _k] = {"hit.%d" % _k, "_falsehit.%d" % _k}
for _q in range(60):
    MUTANT_SCOPE["drop_neighbour_%d" % _q] = {"_write.%d" % _q}
for _k in FLIP_KINDS:
    MUTANT_SCOPE["flip:" + _k] = {_k}


def mutants_of(kind):
    """the mutants that are wrong in `kind` (tests/test_slot_census_cpu.py: each predicts differently on an input built for the kind).  The
    first one decides differently at events of that kind and nowhere else, but for the two kinds of a tag-0 context meeting empty slots,
    which share tag0_is_miss.  A second one, where there is one, is a slip of wider scope (MUTANT_SCOPE) that shows in this kind:
    conf_cap_7 is wrong at any miss with a confidence above 7 (under the cap all four look equal and slot 1 goes), skip_cand_k at any miss
    into victim k, le_for_lt at any tie."""
    if kind.startswith("hit."):
        return ("no_match_" + kind[4:],)
    if kind.startswith("packed."):
        return ("drop_neighbour_" + kind[7:],)
    if kind.startswith("state.pinned"):
        return ("no_self_loop",)
    if kind == "miss.tie.tag0_entrant":
        return ("tags_0_to_3", "le_for_lt")
    if kind.endswith(".conf8") and ("victim0" in kind or "victim2" in kind or "victim3" in kind or "0eq2" in kind or "2eq3" in kind):
        return ("flip:" + kind, "conf_cap_7")
    if "victim" in kind and not kind.endswith(".conf8"):
        return ("flip:" + kind, "skip_cand_" + kind[11])
    if kind in FLIP_KINDS:
        return ("flip:" + kind,)
    return ({"falsehit": "full_hash", "tag0.empty_cell": "tag0_is_miss", "tag0.slot3_empty_others_owned": "tag0_is_miss", "miss.tag0": "tag0_miss_no_clear",
             "evict.return": "no_clear_on_evict"}[kind],)


def _nz3(v):
    return (v & 0xF) and (v & 0xF0) and (v & 0xF00)


class _Cell:
    __slots__ = ("tags", "st", "owner", "gone", "tok_self", "tok_nb", "via0")

    def __init__(self):
        self.tags, self.st, self.owner, self.gone = [0] * 4, [0] * 60, [None] * 4, set()
        self.tok_self, self.tok_nb = [None] * 60, [None] * 60
        self.via0 = [False] * 4          # (the slot's context came in as a tag-0 hit on the empty slot)


Event = collections.namedtuple("Event", "cell tag nib slot kinds p")


def events(block, order, log_cells, mutant=None):
    """-> [Event(cell, tag, nibble, slot id, kind names, the four predictions)] of the block's nibble events.  `mutant`: a deliberately
    wrong model (MUTANTS); its events carry no kinds."""
    b = bytes(block)
    H = hashes(b, order)
    cells = (H >> np.uint64(64 - log_cells)).astype(np.int64).tolist()
    tags = (H & np.uint64(0xFFF)).astype(np.int64).tolist()
    keys = H.tolist()                 # (the finaliser is a bijection: equal hashes are equal contexts)
    tbl = {}
    out = []
    census = mutant is None
    cmp_order = (0, 1, 2, 3) if mutant == "tags_0_to_3" else (3, 2, 1, 0)
    no_match = int(mutant[9:]) if mutant and mutant.startswith("no_match_") else -1
    cand = [k for k in ((0, 1, 2, 3) if mutant == "cand_order_0123" else (1, 0, 2, 3)) if mutant != "skip_cand_%d" % k]
    drop = int(mutant[15:]) if mutant and mutant.startswith("drop_neighbour_") else -1
    flip = mutant[5:] if mutant and mutant.startswith("flip:") else None
    for e in range(len(keys)):
        cell, tag, h = cells[e], tags[e], keys[e]
        nib = (b[e >> 1] >> 4) if not e & 1 else (b[e >> 1] & 15)
        C = tbl.get(cell)
        if C is None:
            C = tbl[cell] = _Cell()
        kinds = []
        sid = -1
        for k in cmp_order:
            if C.tags[k] == tag and k != no_match:
                sid = k
                break
        if sid >= 0 and C.owner[sid] is None and mutant == "tag0_is_miss":
            sid = -1
        if sid >= 0 and C.owner[sid] is not None and C.owner[sid] != h and mutant == "full_hash":
            sid = -1
        if sid >= 0:
            own = C.owner[sid]
            if own == h:
                kinds.append("hit.%d" % sid)
            elif own is not None:
                kinds += ["falsehit", "_falsehit.%d" % sid]
            else:                                  # an empty slot: its tag is 0, and so is the context's
                kinds.append("_tag0.empty_slot")
                if sid < 3:
                    kinds.append("tag0.hit_empty_below_3")
                elif not any(o is not None for o in C.owner):
                    kinds.append("tag0.empty_cell")
                elif all(C.owner[k] is not None for k in (0, 1, 2)):
                    kinds.append("tag0.slot3_empty_others_owned")
                C.owner[sid], C.via0[sid] = h, True
        else:
            conf = [CONF[C.st[15 * k]] for k in range(4)]
            cc = [min(c, 7) for c in conf] if mutant == "conf_cap_7" else conf
            best = 256
            for k in cand:
                if cc[k] < best or (mutant == "le_for_lt" and cc[k] <= best):
                    best, sid = cc[k], k
            others = [conf[k] for k in range(4) if k != sid]
            named = []
            if all(conf[sid] < x for x in others):
                named.append("miss.victim%d.strict" % sid)
            elif census:
                kinds.append("_miss.tie")
            if conf[0] == conf[1] == conf[2] == conf[3]:
                named.append("miss.tie.all4_to_1")
            elif sid == 0 and conf[2] == conf[0]:
                named.append("miss.tie.0eq2_to_0")
            elif sid == 2 and conf[3] == conf[2]:
                named.append("miss.tie.2eq3_to_2")
            elif sid == 1 and sum(x == conf[1] for x in others) == 1:
                named.append("miss.tie.1_and_one_later_to_1")
            if min(conf) >= 8:
                named += [k + ".conf8" for k in named]
            if min(conf) >= 20 and "miss.tie.all4_to_1" in named:
                named.append("miss.tie.all4.conf20")
            if census:
                kinds += named
                if max(conf) > 7:
                    kinds.append("_miss.conf_gt7")
                kinds.append("_miss.victim%d" % sid)
                if tag == 0:
                    kinds.append("miss.tag0")
                if sum(x == min(conf) for x in conf) > 1 and any(C.via0[k] and conf[k] == min(conf) for k in range(4)):
                    kinds.append("miss.tie.tag0_entrant")
                if C.owner[sid] is not None:
                    kinds.append("_evict.live")
                if h in C.gone:
                    kinds.append("evict.return")
            elif flip in named:
                sid = max((k for k in (1, 0, 2, 3) if k != sid), key=lambda k: (conf[k], (1, 0, 2, 3).index(k)))
            if C.owner[sid] is not None:
                C.gone.add(C.owner[sid])
            C.gone.discard(h)
            C.tags[sid], C.owner[sid], C.via0[sid] = tag, h, False
            if not (mutant == "no_clear_on_evict" or (mutant == "tag0_miss_no_clear" and tag == 0)):
                for q in range(15 * sid, 15 * sid + 15):
                    C.st[q] = 0
                    C.tok_self[q] = C.tok_nb[q] = None
        p = []
        ctx = 0
        for bit_id in range(4):
            bit = (nib >> (3 - bit_id)) & 1
            q = 15 * sid + (1 << bit_id) - 1 + ctx
            s = C.st[q]
            p.append(PROB[s])
            ns = NEXT1[s] if bit else NEXT0[s]
            if census:
                if s == PIN0 and not bit:
                    kinds.append("state.pinned_949")
                if s == PIN1 and bit:
                    kinds.append("state.pinned_3962")
                kinds.append("_write.%d" % q)
                # packed-state stress at q: the write below puts a state of three non-zero nibbles between two non-zero neighbours, and both
                # q and the neighbour it shares a byte with are read again before anything clears them
                for t in (C.tok_self[q], C.tok_nb[q]):
                    if t is not None:
                        t[0 if t is C.tok_self[q] else 1] = True
                        if t[0] and t[1] and not t[2]:
                            t[2] = True
                            kinds.append("packed.%d" % t[3])
                C.tok_self[q] = C.tok_nb[q] = None
                r = q + 1 if q % 2 == 0 else q - 1
                if _nz3(ns) and (q == 0 or C.st[q - 1]) and (q == 59 or C.st[q + 1]) and ((C.st[r] >> 8) if r > q else (C.st[r] & 15)):
                    t = [False, False, False, q]
                    C.tok_self[q], C.tok_nb[r] = t, t
            elif mutant == "no_self_loop":
                if s == PIN0 and not bit:
                    ns = NEXT0[s + 1]
                if s == PIN1 and bit:
                    ns = NEXT1[s - 1]
            C.st[q] = ns
            if q == drop:                          # the write of q takes the neighbour's nibble in the shared byte with it
                if q % 2 == 0:
                    C.st[q + 1] &= 0x0FF
                else:
                    C.st[q - 1] &= 0xFF0
            ctx = (ctx << 1) | bit
        out.append(Event(cell, tag, nib, sid, tuple(kinds), tuple(p)))
    return out


def predict(block, order, log_cells, mutant=None):
    """-> the 8 * len probabilities, in step order"""
    ev = events(block, order, log_cells, mutant)
    return np.array([x for e in ev for x in e.p], dtype=np.uint16)


def pipeline_kinds(ev):
    """k_slot's cases of every event e, by the parity of e and by whether e evicted"""
    st = collections.Counter()
    c = [e.cell for e in ev]
    n = len(c)
    if n in (2, 4, 6):
        st["pipe.block_of_%d" % (n // 2)] += 1
    for e in range(n):
        sfx = ".%s.%s" % ("odd" if e & 1 else "even", "evict" if any(k.startswith("_miss.victim") for k in ev[e].kinds) else "plain")
        prev = c[e - 1] if e else -1
        if e + 1 < n:
            st["pipe." + ("next_same" if c[e + 1] == c[e] else "next_is_prev" if c[e + 1] == prev else "next_other") + sfx] += 1
        if e + 2 < n and c[e + 1] != c[e]:
            if c[e + 2] == c[e]:
                st["pipe.e2_same" + sfx] += 1
            elif c[e + 2] == prev and c[e + 1] != prev:
                st["pipe.e2_is_prev" + sfx] += 1
    return st


def layout_kinds(data, order, log_cells, block_size):
    """the cases of k_slot that take several lanes: `data` in blocks of block_size, 64 blocks per wavefront"""
    st = collections.Counter()
    blocks = [data[o:o + block_size] for o in range(0, len(data), block_size)]
    if len(blocks) % 64:
        st["layout.mirrored_lanes"] += 1
    for w in range(0, len(blocks), 64):
        lens = [len(x) for x in blocks[w:w + 64]] + [0] * (64 - len(blocks[w:w + 64]))
        if len(set(lens)) > 1:
            st["layout.unequal_lanes"] += 1
        cs = [cells_of(x, order, log_cells) for x in blocks[w:w + 64]]
        nev = max(2 * x for x in lens)
        some = np.zeros(nev, dtype=bool)
        other = np.zeros(nev, dtype=bool)
        for c in cs:
            if len(c) > 2:
                same = c[2:] == c[:-2]
                some[:len(same)] |= same
                other[:len(same)] |= ~same
        st["layout.e2_same_some_lanes"] += int((some & other).sum())
        if sum(1 for x in lens if x) > 1:             # (a lone lane has such steps all the time)
            st["layout.e2_same_none_then_some"] += int((~some[:-1] & some[1:]).sum())
    return +st


def leaf_w(log_cells):
    return min(4, max(1, min(1 << log_cells, 1024) // 64))


def lane_ranges(ev, log_cells):
    """-> per lane of the leaf's 64 * leaf_w: the indices of its events, sorted stably by Cell"""
    W = leaf_w(log_cells)
    sh2 = max(log_cells - 10, 0)
    nbins = 1 << (log_cells - sh2)
    cell = np.array([e.cell for e in ev], dtype=np.int64)
    order = np.argsort(cell, kind="stable")
    fine = cell[order] >> sh2
    out = []
    for L in range(64 * W):
        lo, hi = L * nbins // (64 * W), (L + 1) * nbins // (64 * W)
        out.append(order[np.searchsorted(fine, lo, "left"):np.searchsorted(fine, hi, "left")] if hi > lo else order[:0])
    return out


def replay_kinds(ev, log_cells):
    st = collections.Counter()
    W = leaf_w(log_cells)
    st["replay.leaf_w%d" % W] += 1
    sh2 = max(log_cells - 10, 0)
    if (1 << (log_cells - sh2)) < 64 * W:
        st["replay.fewer_bins_than_lanes"] += 1
    if sh2:
        st["replay.cells_share_a_bin"] += 1
    st["replay.two_passes" if log_cells > 8 else "replay.one_pass"] += 1
    if len(ev) in (2046, 2048, 2050):
        st["replay.tile_%d" % len(ev)] += 1
    lanes = lane_ranges(ev, log_cells)
    for w in range(W):
        counts = [len(r) for r in lanes[64 * w:64 * w + 64]]
        maxc = max(counts)
        if maxc and min(counts) == 0:
            st["replay.idle_lane_beside_busy"] += 1
        if maxc == len(ev) and len(ev):
            st["replay.one_lane_has_all"] += 1
        for cnt in counts:
            if cnt in (1, 7, 8, 9, 16):
                st["replay.count_%d" % cnt] += 1
            if 0 < cnt < maxc:
                st["replay.count_below_maxc"] += 1
    for r in lanes:
        cur, valid, evicted = -1, set(), set()
        for k, e in enumerate(r.tolist()):
            x = ev[e]
            if x.cell != cur:
                if k:
                    st["replay.cell_change_at_chunk_start" if k % 8 == 0 else "replay.cell_change_mid_chunk"] += 1
                cur, valid, evicted = x.cell, set(), set()
            miss = any(kk.startswith("_miss.victim") for kk in x.kinds)
            if miss and x.slot in valid:
                evicted.add(x.slot)
            elif not miss and x.slot in evicted:
                st["replay.evict_then_reuse"] += 1
            if x.slot not in valid and valid:
                st["replay.slot_first_touched_after_another"] += 1
            valid.add(x.slot)
    return +st


def kinds(block, order, log_cells, nblocks_layout=1, block_size=512):
    """-> Counter of the kind names that `block` reaches as one block of a leaf (CELL, PIPELINE, REPLAY), or, with nblocks_layout > 1, that
    it reaches as nblocks_layout blocks of block_size (LAYOUT)"""
    if nblocks_layout > 1:
        assert (len(block) + block_size - 1) // block_size == nblocks_layout
        return layout_kinds(block, order, log_cells, block_size)
    ev = events(block, order, log_cells)
    st = collections.Counter(k for e in ev for k in e.kinds)
    return st + pipeline_kinds(ev) + replay_kinds(ev, log_cells)


def describe(block, order, log_cells, step):
    """step (8 i + 4 h + k) -> its event and what the model says of it"""
    ev = events(block, order, log_cells)
    e = step >> 2
    x = ev[e]
    c = [y.cell for y in ev]
    near = " ".join("c[e%+d]=%d" % (d, c[e + d]) for d in (-1, 1, 2) if 0 <= e + d < len(c))
    return ("step %d = bit %d of event %d (byte %d, nibble %d = 0x%x): SlotModel(%d, %d) Cell %d tag 0x%03x slot %d, predictions %s, kinds [%s]; %s"
            % (step, step & 3, e, e >> 1, e & 1, x.nib, order, log_cells, x.cell, x.tag, x.slot, list(x.p),
               " ".join(k for k in x.kinds if not k.startswith("_write")), near))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def alphabet_block(seed, letters, n):
    """n bytes drawn evenly from a random alphabet of `letters` byte values"""
    rng = np.random.default_rng(seed)
    a = rng.permutation(256)[:letters].astype(np.uint8)
    return a[rng.integers(0, letters, n)].tobytes()


def shared_cell_letters(log_cells, seed, letters):
    """byte values whose order-1 first-nibble contexts fall into one Cell of a leaf of 2^log_cells Cells (the fullest one), tags distinct"""
    x = np.arange(256, dtype=np.uint64)
    h = context_hash(1, x, np.zeros(256, dtype=np.uint64))
    cell = (h >> np.uint64(64 - log_cells)).astype(np.int64)
    full = np.bincount(cell).argmax()
    cand = np.flatnonzero(cell == full)
    _, first = np.unique(h[cand] & np.uint64(0xFFF), return_index=True)
    cand = cand[np.sort(first)]
    return np.random.default_rng(seed).permutation(cand)[:letters].astype(np.uint8)


def shared_cell_runs(seed, log_cells, letters, lead, lengths, n=4096):
    """runs of equal bytes over shared_cell_letters: `letters` contexts compete for the four slots of one Cell, each with as many
    observations as its runs are long.  The block opens with one run of `lead` bytes per letter (four equal confidences, then a fifth
    context), and goes on with runs of lengths drawn from `lengths`."""
    rng = np.random.default_rng(seed)
    a = shared_cell_letters(log_cells, seed, letters)
    out = [np.repeat(a, lead)]
    left = n - lead * len(a)
    while left > 0:
        r = int(rng.choice(lengths))
        out.append(np.repeat(a[rng.integers(0, len(a))], r))
        left -= r
    return np.concatenate(out)[:n].tobytes()


def tag0_pairs(log_cells):
    """(y, x, Cell) of the order-2 first-nibble contexts "y then x" whose tag is 0"""
    yx = np.arange(65536, dtype=np.uint64)
    h = context_hash(2, yx, np.zeros(65536, dtype=np.uint64))
    hit = np.flatnonzero((h & np.uint64(0xFFF)) == 0)
    return [(int(v) >> 8, int(v) & 255, int(h[v] >> np.uint64(64 - log_cells))) for v in hit]


def tag0_block(seed, log_cells, pairs, others, n):
    """an order-2 block over the letters of `pairs` tag-0 contexts and `others` random ones.  It opens with the first pair, whose
    context then meets its Cell before anything else has (if the search over seeds says so), and goes on evenly at random."""
    rng = np.random.default_rng(seed)
    t0 = tag0_pairs(log_cells)
    pick = [t0[int(k)] for k in rng.permutation(len(t0))[:pairs]]
    a = np.array(sorted({v for y, x, _ in pick for v in (y, x)} | set(rng.permutation(256)[:others].tolist())), dtype=np.uint8)
    body = a[rng.integers(0, len(a), n)]
    # every pair in a row now and then, so that its context comes up more often than chance has it
    for k in range(8, n - 2, 24):
        y, x, _ = pick[int(rng.integers(0, len(pick)))]
        body[k], body[k + 1] = y, x
    body[0], body[1] = pick[0][0], pick[0][1]
    return body.tobytes()


# name -> (bytes, order, log_cells); every block at most 4,096 bytes.  The seeds come from a search over the census above: each was
# kept for the kinds it adds (tests/test_slot_census_cpu.py prints which input reaches which kind, and pins the bytes).
SMALL_INPUTS = {
    "alphabet12_cells4": (lambda: alphabet_block(1, 12, 4096), 1, 2),
    "alphabet12_cells4_b": (lambda: alphabet_block(2, 12, 4096), 1, 2),
    "runs_shared_cell": (lambda: shared_cell_runs(0, 4, 7, 50, (50, 12, 12, 9, 3)), 1, 4),
    "runs_shared_cell_b": (lambda: shared_cell_runs(3, 4, 6, 12, (8, 10, 10, 12, 12, 16)), 1, 4),
    "tag0": (lambda: tag0_block(21, 4, 3, 3, 2048), 2, 4),
    "tag0_b": (lambda: tag0_block(2, 2, 3, 3, 2048), 2, 2),
    # a tag-0 context takes slot 3 of a Cell that still has empty slots, and later shares the least confidence with a neighbour: the
    # narrowest input on which <= for < and the tags compared 0 .. 3 predict differently (the first hit of a search over seeds and sizes)
    "tag0_entrant_tie": (lambda: tag0_block(24, 1, 1, 2, 256), 2, 1),
    "random_cells64": (lambda: alphabet_block(4, 256, 4096), 1, 6),
    "random_cells128": (lambda: alphabet_block(5, 256, 4096), 1, 7),
    "alphabet40_cells4096": (lambda: alphabet_block(6, 40, 4096), 2, 12),
    "alphabet8_cells16": (lambda: alphabet_block(7, 8, 4096), 1, 4),
    "alphabet5_cells2": (lambda: alphabet_block(9, 5, 4096), 2, 1),
    "tile_2046": (lambda: alphabet_block(11, 20, 1023), 2, 8),
    "tile_2048": (lambda: alphabet_block(12, 256, 1024), 2, 9),
    "tile_2050": (lambda: alphabet_block(13, 30, 1025), 3, 10),
    "zeros": (lambda: bytes(300), 1, 2),
    "ff": (lambda: b"\xff" * 300, 1, 2),
    "one_cell": (lambda: b"\x10" * 64, 0, 1),        # (both contexts of the block in Cell 0 of two)
    "block_of_1": (lambda: b"\x5a", 1, 2),
    "block_of_2": (lambda: b"\x5a\xa5", 1, 2),
    "block_of_3": (lambda: b"\xa5\x5a\xa5", 2, 4),
}
# the inputs whose 65-block layout (layout_of) the GPU test runs: between them they reach every PIPELINE and LAYOUT kind
PIPELINE_INPUTS = ("alphabet12_cells4", "random_cells64")
_cache = {}


def block(name):
    """the named input, made once -> (bytes, order, log_cells)"""
    if name not in _cache:
        mk, order, log_cells = SMALL_INPUTS[name]
        _cache[name] = (mk(), order, log_cells)
    return _cache[name]


def block_events(name):
    if ("ev", name) not in _cache:
        _cache[("ev", name)] = events(*block(name))
    return _cache[("ev", name)]


def block_kinds(name):
    if ("kinds", name) not in _cache:
        ev = block_events(name)
        _cache[("kinds", name)] = collections.Counter(k for e in ev for k in e.kinds) + pipeline_kinds(ev) + replay_kinds(ev, block(name)[2])
    return _cache[("kinds", name)]


def layout_of(name, nblocks=65, block_size=512, tail=77):
    """the named input as nblocks blocks: block j is the input rotated by 7 j bytes and cut to block_size, the last one to `tail`"""
    data = np.frombuffer(block(name)[0], dtype=np.uint8)
    parts = [np.roll(data, -7 * j)[:block_size] for j in range(nblocks)]
    parts[-1] = parts[-1][:tail]
    return np.concatenate(parts).tobytes()
