"""A CPU model of which states of an APM stage, of k_apm0's and k_apm1's schedules and of the leaf mixer one block reaches, and the
inputs built to reach every one of them: test infrastructure, no device code.  tests/test_apm_census_cpu.py checks the model against
the oracle step for step, asserts that the inputs reach the states and that a model wrong in one behaviour predicts differently;
tests/test_gpu_apm_states.py runs the same bytes through the kernels.

What is restated here:

The stage (oracle/w3_oracle.c apm_pp :1117-1126, apm_update :1127-1136, apm_reset :1104-1108, the tables ss_build :1075-1094).  Step
8 i + j is bit j (most significant first) of byte i.  The row is c0 = (1 << j) | (byte >> (8 - j)) for W3_APM_ORDER0 and c0 | c1 << 8
for W3_APM_ORDER1, c1 = the byte before, 0 at the block start.  pos = (stretch(p) + 2048) * 32, j' = pos >> 12, w = pos & 4095;
pa = (t[j'] (4096 - w) + t[j' + 1] w) >> 12; out = clamp((p + 3 pa + 2) >> 2, 1, 65535); the entry j' + (w >> 11) moves towards
65535 * bit by floor(delta / 2^rate).  A row starts as squash(clip((e - 16) * 128, -2047, 2047)), e = 0 .. 32.  stretch lies in
[-2047, 2047], so j' <= 31 and w is a multiple of 32 from 32 (at j' = 0) to 4064 (at j' = 31).

The kernels' form of a step (weath3rb0i_amd/csrc/w3_apm.h apm_lut_entry :135-139, apm0_prep :149-166, apm0_commit :168-197,
apm0_finish :199-204): the entry trained (`upd`), the other one of the pair (`oth`: the one above when w < 2048, the one below
otherwise) and the weight x = the distance of pos from `upd` in 1/128 of an entry; pa = au + ((ao - au) x >> 7), arithmetic shift;
the update is (old (2^rate - 1) + 65535 bit) >> rate.  Both equal the oracle's forms (the model asserts it at every step).

k_apm0<L> (w3_apm.h :214-357): a block's positions in batches of 32 = 4 rounds of 8; the block's two wavefronts take alternate
batches and hand the table over through `turn` (:279-289).  In a round lane 8 k + j is bit j of position k; the positions are
committed in pairs (2 m, 2 m + 1) (:171-187): both lanes read the entries, the later lane takes the earlier one's new value where it
reads the entry the earlier one trains (masks m_u, m_o of :160-164), and where both train one entry the earlier lane leaves the
store to the later one (`sh`).  Lanes past the block's end take no part (:270-275); a block of a multiple of 32 bytes runs the FAST
form (:355).  Four blocks share a workgroup (:345).

k_apm1 (w3_apm.h :359-459) walks the records sorted by the previous byte (tests/rank_census.py records / splits, reused here) in the
64 slices of the block, rounds of 8 records; a round all of whose valid records are in the open group runs apm0_prep / apm0_commit
(:423-428), any other is committed record by record with scalar arithmetic and a fresh table wherever the group changes (:429-452).

The lane kernels and the decoder (w3_cm.h :178-194, :379-395, :494-509; w3_decode_spec.h :288-315) walk the steps in time order with
the oracle's formulas; k_decode_spec's nibble-major table keeps a row at [page * 17 + G][entry][column], G = 0 for the rows of a
byte's first nibble (c0 < 16) and 1 + the high nibble for those of its second (:296-301).

OpinionMixer2 over L leaves (w3_apm.h :240-251, w3_coder.h opinion_mix2 :183-197, w3_device.h pk_opinion_dist / pk_farther_mask
:56-66): two steps per dword; a later leaf takes a half over where its distance from 32768 is strictly larger, so the leftmost leaf
of the largest distance is kept (oracle w3o_opinion_mix :608-613, nested).

Counter leaves (oracle :202-213, :639-661): p = round(2^16 (n1 + 1) / (n0 + n1 + 2)); Order0's context is the bit position and the
last 8 bits, Order1's the bit position and the last 16, OrderN(bits, 3)'s the last bits - 3 bits and the bit position."""
import collections

import numpy as np

from tests import rank_census as rc

ORDER0, ORDER1 = 0, 1


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def _tables():
    K = 0xFF007FD5
    e = 1 << 32
    sq = [0] * 4095
    for d in range(2048):
        den = (1 << 32) + e
        q = min(((1 << 48) + den // 2) // den, 65535)
        sq[2047 + d] = q
        sq[2047 - d] = max(65536 - q, 1)
        e = (e * K) >> 32
    sq[2047] = 32768
    st = []
    d = -2047
    for q in range(4096):
        while d < 2047 and sq[d + 2047] < q * 16 + 8:
            d += 1
        st.append(d)
    return sq, st


SQUASH, STRETCH = _tables()


def squash(d):
    return SQUASH[max(-2047, min(2047, d)) + 2047]


ROW_INIT = [squash((e - 16) * 128) for e in range(33)]
# what a row initialised without the clip would hold: (e - 16) * 128 = -2048 and +2048 lie one entry outside the squash table, whose
# neighbours in memory are unknown; the mutant reads 0 there
ROW_INIT_NO_CLIP = [0] + ROW_INIT[1:32] + [0]


# ---- leaves and the mixer -------------------------------------------------------------------------------------------------------------
_leaf_cache = {}


def leaf_stream(block, leaf):
    """the 8 * len predictions of one Counter leaf: ("o0",), ("o1",) or ("on", bits, align_bits); kept for the blocks of the census"""
    key = (bytes(block), tuple(leaf))
    if key not in _leaf_cache:
        if len(_leaf_cache) > 256:
            _leaf_cache.clear()
        _leaf_cache[key] = _leaf_stream(block, leaf)
    return _leaf_cache[key]


def _leaf_stream(block, leaf):
    kind = leaf[0]
    if kind == "o0":
        hmask, shift = 0xFF, 8
    elif kind == "o1":
        hmask, shift = 0xFFFF, 16
    else:
        hmask, shift = (1 << (leaf[1] - leaf[2])) - 1, None
        abits = leaf[2]
    n0, n1 = collections.defaultdict(int), collections.defaultdict(int)
    out = []
    hist = align = ctx = 0
    for byte in bytes(block):
        for j in range(8):
            bit = (byte >> (7 - j)) & 1
            a, b = n0[ctx], n1[ctx]
            p = (1 << 17) * (b + 1) // (a + b + 2)
            out.append((p >> 1) + (p & 1))
            if bit:
                n1[ctx] = b + 1
            else:
                n0[ctx] = a + 1
            if n0[ctx] == 0xFFFF or n1[ctx] == 0xFFFF:
                n0[ctx], n1[ctx] = (n0[ctx] >> 1) + (n0[ctx] & 1), (n1[ctx] >> 1) + (n1[ctx] & 1)
            hist = ((hist << 1) | bit) & hmask
            if shift is not None:
                align = (align + 1) % 8
                ctx = (align << shift) | hist
            else:
                align = (align + 1) & ((1 << abits) - 1)
                ctx = (hist << abits) | align
    return out


MIX_KINDS2 = ["mix.farther_low_only", "mix.farther_high_only", "mix.farther_both", "mix.farther_neither", "mix.tie_same_side",
              "mix.tie_opposite_sides", "mix.both_at_half"]
MIX_KINDS3 = ["mix.third_beats_winner", "mix.three_tied_leftmost_kept"]
MIX_MUTANTS = ["mix_tie_right", "mix_cross_halves"]


def mix(streams, mutant=None, kinds=None):
    """OpinionMixer2 over the leaves' streams, two steps per dword as the kernels do it -> the mixed stream.  `kinds`: a Counter that
    receives the mixer's state names, or a list that receives (step, name)."""
    if len(streams) == 1:
        return list(streams[0])
    n = len(streams[0])
    w = list(streams[0])
    d = [abs(p - 32768) for p in w]
    note = None
    if kinds is not None:
        note = (lambda s, k: kinds.append((s, k))) if isinstance(kinds, list) else (lambda s, k: kinds.update((k,)))
    first_tied = None
    for li in range(1, len(streams)):
        q = streams[li]
        e = [abs(p - 32768) for p in q]
        if mutant == "mix_tie_right":
            far = [e[s] >= d[s] for s in range(n)]
        else:
            far = [e[s] > d[s] for s in range(n)]
        if note:
            for s in range(0, n, 2):
                lo, hi = far[s], far[s + 1]
                note(s, "mix.farther_" + ("both" if lo and hi else "low_only" if lo else "high_only" if hi else "neither"))
            for s in range(n):
                if e[s] == d[s]:
                    if e[s] == 0:
                        note(s, "mix.both_at_half")
                    elif q[s] == w[s]:
                        note(s, "mix.tie_same_side")
                    else:
                        note(s, "mix.tie_opposite_sides")
            if li == 1:
                first_tied = [e[s] == d[s] for s in range(n)]
            if li == 2:
                for s in range(n):
                    if far[s]:
                        note(s, "mix.third_beats_winner")
                    elif first_tied[s] and e[s] == d[s]:
                        note(s, "mix.three_tied_leftmost_kept")
        if mutant == "mix_cross_halves":         # the low half's compare decides the high half and the other way round
            far = [far[s ^ 1] for s in range(n)]
        for s in range(n):
            if far[s]:
                w[s] = q[s]
            if e[s] > d[s]:
                d[s] = e[s]
    return w


# ---- (a) one stage, step by step ------------------------------------------------------------------------------------------------------
LOOKUP_KINDS = (["stretch.-2047", "stretch.+2047", "w.0", "w.2048", "w.2016", "w.32", "w.4064"]
                + ["entry.%d.bit%d" % (e, b) for e in range(33) for b in (0, 1)])
INTERP_KINDS = ["interp.other_below_inexact", "interp.other_above_inexact", "interp.neighbours_equal"]
UPDATE_KINDS = ["update.negative_inexact", "update.arrives_at_0", "update.stays_0", "update.leaves_0", "update.stall"]
OUTPUT_KINDS = ["out.low_clamp"]
ROW0_KINDS = ["row.%d" % r for r in range(1, 256)]
ROW1_KINDS = ["row.c1_0_at_start", "row.revisited_after_another_page", "row.group_0", "row.group_1_plus_h"]
STAGE_MUTANTS = ["update_truncates", "interp_truncates", "tie_to_lower", "no_low_clamp", "init_no_clip", "order1_c1_is_current"]

Prep = collections.namedtuple("Prep", "p upd oth x bit kinds")


def prep(p_in, block, kind, mutant=None):
    """what a step needs that does not depend on the table: the entry trained and the other one (row * 33 + entry), the weight of
    the other one in 1/128, the bit, and the names of the step's lookup and row states"""
    b = bytes(block)
    upd, oth, xs, bits, kinds = [], [], [], [], []
    c1 = 0
    seen_rows, last_page = set(), None
    for i, byte in enumerate(b):
        page = c1 if kind == ORDER1 else 0
        if mutant == "order1_c1_is_current" and kind == ORDER1:
            page = byte
        for j in range(8):
            s = 8 * i + j
            c0 = (1 << j) | (byte >> (8 - j))
            bit = (byte >> (7 - j)) & 1
            p = p_in[s]
            st = STRETCH[p >> 4]
            pos = (st + 2048) * 32
            jj, w = pos >> 12, pos & 4095
            hi = w >> 11
            if mutant == "tie_to_lower" and w == 2048:
                hi = 0
            row = c0 | (page << 8)
            u = jj + hi
            o = jj + 1 - hi
            x = (w >> 5) if not hi else ((4096 - w) >> 5)
            upd.append(row * 33 + u)
            oth.append(row * 33 + o)
            xs.append(x)
            bits.append(bit)
            k = ["entry.%d.bit%d" % (u, bit)]
            if st == -2047:
                k.append("stretch.-2047")
            if st == 2047:
                k.append("stretch.+2047")
            if w in (0, 2048, 2016, 32, 4064):
                k.append("w.%d" % w)
            if kind == ORDER0:
                k.append("row.%d" % c0)
            else:
                if i == 0:
                    k.append("row.c1_0_at_start")
                k.append("row.group_0" if c0 < 16 else "row.group_1_plus_h")
                if row in seen_rows and last_page != page:
                    k.append("row.revisited_after_another_page")
            kinds.append(k)
        if kind == ORDER1:
            for j in range(8):
                seen_rows.add(((1 << j) | (byte >> (8 - j))) | (page << 8))
            last_page = page
        c1 = byte
    return Prep(list(p_in), upd, oth, xs, bits, kinds)


def _nv(old, bit, rate, mutant=None):
    delta = (65535 if bit else 0) - old
    if mutant == "update_truncates":
        return old + (delta >> rate if delta >= 0 else -((-delta) >> rate))
    nv = (old * ((1 << rate) - 1) + (65535 if bit else 0)) >> rate           # the kernels' form
    assert nv == old + (delta >> rate)                                        # the oracle's floor
    return nv


def _finish(p, au, ao, x, mutant=None):
    prod = (ao - au) * x
    if mutant == "interp_truncates":
        pa = au + (prod >> 7 if prod >= 0 else -((-prod) >> 7))
    else:
        pa = au + (prod >> 7)
    o = (p + 3 * pa + 2) >> 2
    assert o <= 65535, "the high clamp cannot fire: (65535 * 4 + 2) >> 2 = 65535"
    if o < 1 and mutant != "no_low_clamp":
        o = 1
    return o, pa


def _dyn_kinds(p, au, ao, x, bit, nv, rate, pa, k):
    prod = (ao - au) * x
    if ao == au:
        k.append("interp.neighbours_equal")
    elif prod & 127:
        k.append("interp.other_below_inexact" if ao < au else "interp.other_above_inexact")
    delta = (65535 if bit else 0) - au
    if delta < 0 and (-delta) & ((1 << rate) - 1):
        k.append("update.negative_inexact")
    if au == 0:
        k.append("update.leaves_0" if bit else "update.stays_0")
    elif nv == 0:
        k.append("update.arrives_at_0")
    if 0 < delta < (1 << rate):
        k.append("update.stall")
    if p == 1 and pa == 0:
        k.append("out.low_clamp")


def _row(mutant):
    return ROW_INIT_NO_CLIP if mutant == "init_no_clip" else ROW_INIT


def stage(p_in, block, kind, rate, mutant=None, with_kinds=True):
    """one APM stage in time order -> (output stream, per step the list of its state names)"""
    q = prep(p_in, block, kind, mutant)
    row = _row(mutant)
    t = {}
    out = []
    for s in range(len(q.p)):
        u, o = q.upd[s], q.oth[s]
        au = t.get(u)
        if au is None:
            au = row[u % 33]
        ao = t.get(o)
        if ao is None:
            ao = row[o % 33]
        if mutant is None:        # the oracle's interpolation over (j', w) is the kernels' over (upd, oth, x)
            lo, hi_ = (au, ao) if o > u else (ao, au)
            w = (q.x[s] << 5) if o > u else 4096 - (q.x[s] << 5)
            assert (lo * (4096 - w) + hi_ * w) >> 12 == au + (((ao - au) * q.x[s]) >> 7)
        nv = _nv(au, q.bit[s], rate, mutant)
        t[u] = nv
        res, pa = _finish(q.p[s], au, ao, q.x[s], mutant)
        out.append(res)
        if with_kinds:
            _dyn_kinds(q.p[s], au, ao, q.x[s], q.bit[s], nv, rate, pa, q.kinds[s])
    return out, q.kinds


# ---- (b) k_apm0's schedule ------------------------------------------------------------------------------------------------------------
PAIR_KINDS = ["pair.same_entry", "pair.later_other_is_earlier_trained", "pair.later_trained_is_earlier_other", "pair.same_row_disjoint",
              "pair.different_rows"]
FORWARD_KINDS = [k + v for k in PAIR_KINDS[:2] for v in (".value_0", ".value_stalls")]
BOUNDARY_KINDS = ["dep.across_substep", "dep.across_round", "dep.across_batch"]
SHAPE_KINDS = (["shape.fast", "shape.last_pair_earlier_only", "shape.empty_round"] + ["shape.nbatch_%d" % k for k in range(1, 8)]
               + ["shape.blocks_1", "shape.blocks_4", "shape.blocks_5"])
SCHED_MUTANTS = ["stale_same_entry", "stale_other_entry", "earlier_store_wins", "forward_on_earlier_other", "batch_handover_lost"]


def _pair(t, row, q, sE, sL, rate, mutant, out, kinds, prefix="pair."):
    """one lane pair of a sub-step: steps sE (earlier position) and sL (later position, or None when it lies past the end)"""
    def rd(i):
        v = t.get(i)
        return row[i % 33] if v is None else v
    uE, oE = q.upd[sE], q.oth[sE]
    auE, aoE = rd(uE), rd(oE)
    tE = _nv(auE, q.bit[sE], rate)
    out[sE] = _finish(q.p[sE], auE, aoE, q.x[sE])[0]
    if sL is None:
        t[uE] = tE
        return
    uL, oL = q.upd[sL], q.oth[sL]
    auL, aoL = rd(uL), rd(oL)
    same, other = uE == uL, uE == oL
    if same and mutant != "stale_same_entry":
        auL = tE
    if other and mutant != "stale_other_entry":
        aoL = tE
    if mutant == "forward_on_earlier_other" and oE == uL and not same:
        auL = tE
    tL = _nv(auL, q.bit[sL], rate)
    out[sL] = _finish(q.p[sL], auL, aoL, q.x[sL])[0]
    if same and mutant == "earlier_store_wins":
        t[uE] = tE
    else:
        if not same:
            t[uE] = tE
        t[uL] = tL
    if kinds is not None:
        if same:
            k = "same_entry"
        elif other:
            k = "later_other_is_earlier_trained"
        elif uL == oE:
            k = "later_trained_is_earlier_other"
        elif uE // 33 == uL // 33:
            k = "same_row_disjoint"
        else:
            k = "different_rows"
        kinds[sL].append(prefix + k)
        if same or other:
            if tE == 0:
                kinds[sL].append(prefix + k + ".value_0")
            if q.bit[sE] and tE == auE:
                kinds[sL].append(prefix + k + ".value_stalls")


def apm0_schedule(p_in, block, rate, mutant=None, with_kinds=True):
    """an ORDER0 stage in k_apm0's order -> (output stream, per step the names of its pair and boundary states)"""
    q = prep(p_in, block, ORDER0)
    n = len(bytes(block))
    out = [0] * (8 * n)
    kinds = [[] for _ in range(8 * n)] if with_kinds else None
    t = {}
    lost = mutant == "batch_handover_lost"
    snaps = []
    for base in range(0, n, 32):
        bi = base // 32
        if lost:
            snaps.append(dict(t))
        tt = dict(snaps[bi - 1]) if lost and bi >= 1 else t       # the table as the batch before this one found it
        written = {}
        for pos in range(base, min(base + 32, n), 2):
            for j in range(8):
                sE = 8 * pos + j
                sL = sE + 8 if pos + 1 < n else None
                _pair(tt, ROW_INIT, q, sE, sL, rate, mutant, out, kinds)
                if tt is not t:
                    written[q.upd[sE]] = tt[q.upd[sE]]
                    if sL is not None:
                        written[q.upd[sL]] = tt[q.upd[sL]]
        if tt is not t:
            t.update(written)
    if with_kinds:
        for pos in range(n - 1):
            if pos % 2 == 1:
                for j in range(8):
                    if q.upd[8 * pos + j] == q.upd[8 * pos + 8 + j]:
                        kinds[8 * pos + 8 + j].append("dep.across_batch" if pos % 32 == 31 else "dep.across_round" if pos % 8 == 7
                                                      else "dep.across_substep")
    return out, kinds


def shape_kinds(length, nblocks):
    k = ["shape.blocks_%d" % nblocks] if nblocks in (1, 4, 5) else []
    if length % 32 == 0:
        k.append("shape.fast")
    else:
        if length % 2:
            k.append("shape.last_pair_earlier_only")
        if length % 32 <= 24:
            k.append("shape.empty_round")
    nb = (length + 31) // 32
    if 1 <= nb <= 7:
        k.append("shape.nbatch_%d" % nb)
    return k


# ---- (c) k_apm1's schedule ------------------------------------------------------------------------------------------------------------
APM1_PAIR_KINDS = ["apm1." + k for k in PAIR_KINDS] + ["apm1." + k for k in FORWARD_KINDS]
APM1_PATH_KINDS = ["apm1.fast_round", "apm1.record_by_record_round"]
APM1_CROSS_KINDS = ["apm1.%s:%s" % (path, k) for path in ("fast", "slow") for k in UPDATE_KINDS + OUTPUT_KINDS]
APM1_MUTANTS = ["no_reinit_at_group_change"]


def apm1_schedule(p_in, block, rate, mutant=None, with_kinds=True):
    """an ORDER1 stage in k_apm1's order -> (output stream, per step its path and pair state names, per step "fast" / "slow")"""
    n = len(bytes(block))
    q = prep(p_in, block, ORDER1)
    if mutant == "no_reinit_at_group_change":          # one table for all groups: the rows of every page fall together
        q = q._replace(upd=[u % (256 * 33) for u in q.upd], oth=[o % (256 * 33) for o in q.oth])
    pos, g, _, _ = rc.records(block, "order1")
    pos, g = pos.tolist(), g.tolist()
    sp = rc.splits(np.asarray(g))
    out = [0] * (8 * n)
    kinds = [[] for _ in range(8 * n)] if with_kinds else None
    path = [None] * (8 * n)
    t = {}
    for s in range(rc.SLICES):
        lo, hi = sp[s], sp[s + 1]
        open_g = None
        for base in range(lo, hi, 8):
            rnd = list(range(base, min(base + 8, hi)))
            fast = all(g[r] == open_g for r in rnd)
            for r in rnd:
                for j in range(8):
                    path[8 * pos[r] + j] = "fast" if fast else "slow"
                    if with_kinds:
                        kinds[8 * pos[r] + j].append(APM1_PATH_KINDS[0 if fast else 1])
            if fast:
                for k in range(0, len(rnd), 2):
                    for j in range(8):
                        sE = 8 * pos[rnd[k]] + j
                        sL = 8 * pos[rnd[k + 1]] + j if k + 1 < len(rnd) else None
                        _pair(t, ROW_INIT, q, sE, sL, rate, mutant, out, kinds, "apm1.pair.")
            else:
                for r in rnd:
                    open_g = g[r]            # (the rows of another group are other keys of t: a fresh table)
                    for j in range(8):
                        _pair(t, ROW_INIT, q, 8 * pos[r] + j, None, rate, mutant, out, None)
    return out, kinds, path


# ---- chains ---------------------------------------------------------------------------------------------------------------------------
def form_of(stages, k, nleaves):
    kind = stages[k][0]
    if kind == ORDER0:
        return "order0.first" if k == 0 else "order0.later"
    return "order1.first" if k == 0 else "order1.later"


FORMS = ["order0.first", "order0.later", "order1.first", "order1.later"]
ALL_MUTANTS = STAGE_MUTANTS + SCHED_MUTANTS + APM1_MUTANTS + MIX_MUTANTS


def _applies(mutant, kind):
    if mutant in ("order1_c1_is_current", "no_reinit_at_group_change"):
        return kind == ORDER1
    if mutant == "batch_handover_lost":
        return kind == ORDER0
    return mutant in STAGE_MUTANTS + SCHED_MUTANTS


def chain(block, leaves, stages, mutant=None, engine="time", with_kinds=True, at_stage=None, truth=None):
    """the model (leaf tree, APM stages) over one block -> [the mixed leaf stream, stage 1's stream, ...], [per stage the steps' state
    names].  engine "time": every stage in time order; "schedule": ORDER0 stages in k_apm0's order, ORDER1 stages in k_apm1's.
    `mutant` is applied to the mixer, or to stage `at_stage` (every stage it applies to when None).  `truth`: the true model's streams;
    a mutant's chain then takes them over where it cannot differ and ends with the first stage that differs.  Third result: the
    mixer's (step, name) list."""
    streams = [leaf_stream(block, lf) for lf in leaves]
    mk = [] if with_kinds else None
    p = mix(streams, mutant if mutant in MIX_MUTANTS else None, mk)
    outs, kinds = [p], []
    for k, (kind, rate) in enumerate(stages):
        m = mutant if (at_stage is None or at_stage == k) else None
        if truth is not None:
            if p != truth[k]:
                break
            if not _applies(m, kind):
                outs.append(truth[k + 1])
                p = truth[k + 1]
                continue
        if m in SCHED_MUTANTS + APM1_MUTANTS or engine == "schedule":
            if kind == ORDER0:
                o, kk = apm0_schedule(p, block, rate, m if m in SCHED_MUTANTS else None, with_kinds)
            else:
                o, kk, path = apm1_schedule(p, block, rate, m if m in SCHED_MUTANTS[:4] + APM1_MUTANTS else None, with_kinds)
                if with_kinds:
                    _, tk = stage(p, block, kind, rate)
                    for s in range(len(o)):
                        kk[s] += ["apm1.%s:%s" % (path[s], x) for x in tk[s] if x.startswith("update.") or x.startswith("out.")]
        else:
            o, kk = stage(p, block, kind, rate, m if m in STAGE_MUTANTS else None, with_kinds)
        if with_kinds and k == 0 and mk:
            for s, name in mk:
                kk[s].append(name)
        outs.append(o)
        kinds.append(kk)
        p = o
    return outs, kinds, mk


# ---- (e) inputs -----------------------------------------------------------------------------------------------------------------------
O0, O1 = ("o0",), ("o1",)
SINGLE_BITS = bytes([0x80, 0, 0x40, 0, 0x20, 0, 0x10, 0, 0x08, 0, 0x04, 0, 0x02, 0, 0x01, 0])
MARKERS = (0x80, 0xC0, 0xE0, 0xF0, 0x40, 0x20, 0xA0, 0x60, 0x10, 0x30, 0x50, 0x70, 0x90, 0xB0, 0xD0)


def inverted(b):
    return bytes(255 - x for x in b)


def zeros_then_single_bits():
    """4,400 zero bytes take every Counter of the all-zero history to p <= 15 (stretch = -2047 needs 4,227 visits), then bytes of one
    set bit each train the lowest entries with a 1"""
    return bytes(4400) + SINGLE_BITS * 4


def runs(a, b, n):
    """(a x 00, b x FF) x n: entries driven to 0 and to the stall below 65535, then trained the other way; an odd a puts the end of a run of
    zeros between the two positions of a pair"""
    return (bytes(a) + b"\xff" * b) * n


def marked(body, count=1500, per=8, switch=6, gap=3):
    """`count` bytes of `body` (00 or FF), then units (marker, follow, gap x body) for fifteen markers whose low nibble equals the
    body's: the bytes after a marker are an ORDER1 group of their own, short enough to share a slice with its neighbours, so that
    k_apm1 meets the group's ends inside a round (record by record).  Marker k has per + 3 k units; its first switch + k follows
    are `body`, the rest body ^ 0x0F: the second nibble's rows see entries driven to an end and then trained the other way."""
    out = bytearray(bytes([body]) * count)
    units = []
    for k, m in enumerate(MARKERS):
        mm = m if body == 0 else 255 - m
        for u in range(per + 3 * k):
            units.append((u, k, bytes([mm, body if u < switch + k else body ^ 0x0F]) + bytes([body]) * gap))
    for _, _, unit in sorted(units):
        out += unit
    return bytes(out)


def ramp():
    """every byte value four times, twice in order and twice shuffled: every row of an ORDER0 stage, 256 ORDER1 groups of four"""
    shuffled = np.random.default_rng(1).permutation(256).astype(np.uint8).tobytes()
    return bytes(range(256)) * 2 + shuffled * 2


def alphabet4(seed=13, n=1500):
    """00 and FF (two in five each), 0F and 55 (one in ten each): leaves that disagree, ties on both sides of 1/2"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0x00, 0xFF, 0x0F, 0x55], dtype=np.uint8), n, p=[.4, .4, .1, .1]).tobytes()


def ff_decay():
    """FF x 1808, 00, FF x 386, then (00, FF) x 200: the Counter of bit 0 after FF falls from 1808 : 1 to 12 : 1 one 0 at a time, so a
    first stage trains each of the entries 21 .. 31 with a 0"""
    return b"\xff" * 1808 + b"\x00" + b"\xff" * 386 + b"\x00\xff" * 200


L3 = [O0, O1, ("on", 16, 3)]
L7 = [O0, O1, ("on", 16, 3), ("on", 11, 3), ("on", 19, 3), ("on", 24, 3), ("on", 27, 3)]
# name -> (bytes, leaves, stages = [(context kind, rate)]); every block at most 8 KiB, and at most 4 KiB but for the four that need a
# Counter at p <= 15.  k_decode_spec takes chains of at most two stages.
INPUTS = {
    "zeros_bits.o0": (zeros_then_single_bits, [O0], [(0, 1), (1, 1), (0, 1), (1, 1)]),
    "zeros_bits.o1": (zeros_then_single_bits, [O0, O1], [(1, 1), (0, 1), (1, 1), (0, 1)]),
    "ones_bits.o0": (lambda: inverted(zeros_then_single_bits()), L3, [(0, 1), (1, 1), (0, 1), (1, 1)]),
    "ones_bits.o1": (lambda: inverted(zeros_then_single_bits()), L7, [(1, 1), (0, 1), (1, 1), (0, 1)]),
    "runs41.o0": (lambda: runs(41, 39, 30), [O0, O1], [(0, 2), (0, 3)]),
    "runs41.o1": (lambda: runs(41, 39, 30), [O0], [(1, 2), (1, 3)]),
    "marked0": (lambda: marked(0), [O0], [(0, 1), (0, 1), (0, 1), (1, 1)]),
    "marked1": (lambda: marked(255), [O0], [(0, 1), (0, 1), (0, 1), (1, 1)]),
    "marked0.first": (lambda: marked(0), L3, [(1, 1), (1, 2)]),
    "marked1.first": (lambda: marked(255), [O0, O1], [(1, 1), (0, 2)]),
    "marked1.two": (lambda: marked(255), [O0], [(0, 2), (1, 2)]),
    "ff_decay.o0": (ff_decay, [O0], [(0, 2), (1, 3)]),
    "ff_decay.o1": (ff_decay, [O0], [(1, 2), (0, 3)]),
    "ramp.o0": (ramp, L7, [(0, 7), (0, 15)]),
    "ramp.o1": (ramp, [O0, O1], [(1, 7), (1, 15)]),
    "alphabet4.L7": (alphabet4, L7, [(0, 2), (1, 7)]),
    "alphabet4.L3": (alphabet4, L3, [(0, 3), (0, 2)]),
    "alphabet4.L2": (alphabet4, [O0, O1], [(0, 7)]),
    "alphabet4.o1": (alphabet4, [O0, O1], [(1, 2), (0, 7)]),
}
_cache = {}


def block(name):
    """the named input, made once -> (bytes, leaves, stages)"""
    if name not in _cache:
        mk, leaves, stages = INPUTS[name]
        _cache[name] = (mk(), leaves, stages)
    return _cache[name]


def build(m, leaves, stages):
    """the model as a tree of `m` (the oracle's module or the package): BestOfTwo nested to the left over the leaves, APM stages on top"""
    def leaf(lf):
        return m.Order0() if lf[0] == "o0" else m.Order1() if lf[0] == "o1" else m.OrderN(lf[1], lf[2])
    t = leaf(leaves[0])
    for lf in leaves[1:]:
        t = m.BestOfTwoModel(t, leaf(lf))
    for kind, rate in stages:
        t = m.APM(t, kind, rate)
    return t


# ---- what has to be reached -----------------------------------------------------------------------------------------------------------
_STAGE = LOOKUP_KINDS + INTERP_KINDS + UPDATE_KINDS
_APM0 = ROW0_KINDS + PAIR_KINDS + FORWARD_KINDS + BOUNDARY_KINDS
_APM1 = ROW1_KINDS + APM1_PAIR_KINDS + APM1_PATH_KINDS
# per stage form (ORDER0 / ORDER1, first stage over the leaves / fed by a stage), and per leaf count of an ORDER0 first stage for the mixer
REQUIRED = {
    "order0.first": _STAGE + _APM0,
    "order0.later": _STAGE + OUTPUT_KINDS + _APM0,
    "order1.first": _STAGE + _APM1 + [k for k in APM1_CROSS_KINDS if "low_clamp" not in k],
    "order1.later": _STAGE + OUTPUT_KINDS + _APM1 + APM1_CROSS_KINDS,
    "mix.L2": MIX_KINDS2,
    "mix.L3": MIX_KINDS2 + MIX_KINDS3,
    "mix.L7": MIX_KINDS2 + MIX_KINDS3,
}
FIRST_STAGE_LEAF_COUNTS = (1, 2, 3, 7)
RATES = (1, 2, 7, 15)
# States that no block of the census's size (8 KiB: 8,192 visits of one Counter at the most) reaches, why, and the test that reaches them
# or that nothing does (tests/test_apm_census_cpu.py checks the arithmetic and, through the model, that the 64 KiB zero block reaches the clamp).
UNREACHABLE_SMALL = {
    "order0.first:out.low_clamp": (
        "needs the mixed leaf probability p = 1: a Counter gives round(65536 / (n + 2)) = 1 from n = 43,689 visits with one bit value on",
        "tests/test_gpu_cm.py::test_cm_edge_blocks (zeros64k: 65,536 visits, o012_apm)"),
    "order1.first:out.low_clamp": (
        "as for an ORDER0 first stage: p = 1 needs 43,689 visits",
        "UNCOVERED: no test runs an ORDER1 first stage over a block of 43,689 equal bytes"),
    "second stage:out.low_clamp": (
        "the stage's input (p + 3 pa + 2) >> 2 is 1 only for a leaf p <= 5 = round(65536 / (n + 2)), n >= 11,914 visits; k_decode_spec "
        "takes at most two stages, so in blocks of 8 KiB it never clamps",
        "tests/test_gpu_cm.py::test_cm_edge_blocks (zeros64k, full_cm_small_tables: two stages, decoded by k_decode_spec in its forms)"),
    "out.high_clamp": (
        "(p + 3 pa + 2) >> 2 <= (65535 * 4 + 2) >> 2 = 65535 for p, pa <= 65535: never, in any block; the model asserts it at every step",
        "nothing to cover"),
    "entry at 65535": (
        "an entry moves up by (65535 - t) >> rate, which is 0 from t = 65535 - (2^rate - 1) on, and no row starts above squash(2047) = "
        "%d: the stall below the top (update.stall) is the end state" % SQUASH[4094],
        "nothing to cover"),
}
# k_apm0<L> is instantiated for L = 1 .. 8 from one source; the census reaches every state with L = 1, 2, 3 and 7, and
# tests/test_gpu_apm_states.py runs the mixer input through the other four.

# (input, block length, block count): the shapes of k_apm0's launch, each block a rotation of the input cut to the length, run in
# blocks of that length
SHAPES = [("runs41.o0", 32, 1), ("runs41.o0", 33, 4), ("runs41.o0", 64, 5), ("alphabet4.L7", 95, 1), ("runs41.o0", 128, 4),
          ("alphabet4.L3", 137, 5), ("runs41.o0", 192, 1), ("alphabet4.L7", 200, 4), ("runs41.o0", 224, 5), ("zeros_bits.o0", 7, 5)]


def shape_data(name, length, nblocks):
    data = np.frombuffer(block(name)[0], dtype=np.uint8)
    return np.concatenate([np.roll(data, -13 * j)[:length] for j in range(nblocks)]).tobytes()


def forms(name):
    """the stage form of every stage of the named input, and the key of its mixer states (None unless an ORDER0 first stage mixes)"""
    _, leaves, stages = block(name)
    return [form_of(stages, k, len(leaves)) for k in range(len(stages))], ("mix.L%d" % len(leaves) if stages[0][0] == ORDER0 and len(leaves) > 1 else None)


def block_kinds(name):
    """-> per stage, per step: the state names of both engines (the schedule's and the time order's), made once; both engines' streams
    are asserted equal on the way"""
    if ("kinds", name) not in _cache:
        data, leaves, stages = block(name)
        outs, sk, _ = chain(data, leaves, stages, engine="schedule")
        outs2, tk, _ = chain(data, leaves, stages)
        assert outs == outs2, name
        for k in range(len(stages)):
            for s in range(len(sk[k])):
                sk[k][s] += [x for x in tk[k][s] if not x.startswith("mix.")]
        _cache[("kinds", name)] = sk
        _cache[("streams", name)] = outs
    return _cache[("kinds", name)]


def block_streams(name):
    block_kinds(name)
    return _cache[("streams", name)]


def reached(name):
    """-> {form or mixer key: Counter of state names} of the named input"""
    if ("reached", name) not in _cache:
        fs, mkey = forms(name)
        out = collections.defaultdict(collections.Counter)
        for k, per_step in enumerate(block_kinds(name)):
            for names in per_step:
                for x in names:
                    if x.startswith("mix."):
                        if mkey:
                            out[mkey][x] += 1
                    else:
                        out[fs[k]][x] += 1
        _cache[("reached", name)] = out
    return _cache[("reached", name)]


def describe(name, stage_index, step):
    """the state names of step `step` of stage `stage_index` (0 = the first APM stage) of the named input, for a failure message"""
    data, leaves, stages = block(name)
    kind, rate = stages[stage_index]
    p = block_streams(name)[stage_index][step]
    i, j = divmod(step, 8)
    return ("%s stage %d (%s, rate %d, %s): step %d = bit %d of byte %d (0x%02x after 0x%02x), input p %d, stretch %d, output %d, states [%s]"
            % (name, stage_index, "ORDER1" if kind else "ORDER0", rate, forms(name)[0][stage_index], step, j, i, data[i], data[i - 1] if i else 0,
               p, STRETCH[p >> 4], block_streams(name)[stage_index + 1][step], " ".join(block_kinds(name)[stage_index][step])))
