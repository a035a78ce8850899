// w3_match_spec_plan.h — the match-model leaf's byte-boundary work as a ROW OF SIXTEEN LANES does it (k_decode_spec<.., MATCH>,
// w3_decode_spec.h), in plain C++ for host and device (no HIP header; tests/host/match_row.cpp compiles it with g++ and walks it with
// sixteen simulated lanes against w3_match_plan.h's serial match_advance).  Everything here must equal the serial `c = T[h]; T[h] = i`
// form over the bytes decoded so far; the hash, the compare's bounds, the bucket and the key are w3_match_plan.h's, called from here.
//
// Boundary i + 1 of a block (the bytes [0, i] known once byte i is decoded), by the row that decodes the block:
//   * the context word is the row's bit history: at a byte boundary it is match_window's word (the last eight bytes big-endian, zeros
//     before the block start), so neither hash needs a load;
//   * after the FIRST nibble of byte i the byte has sixteen possible values: lane r hashes its candidate word (history << 4) | r for m
//     and 2m (match_row_word) and reads T_m[h], T_2m[h] — the tables' state after boundary i's store — beside the second nibble's Counter
//     look-ups; after the second nibble the row takes the entries of the lane whose r is the decoded LOW nibble (match_row_is_writer),
//     and only that lane stores i + 1;
//   * the boundary side of match_length's compare, bytes i-31 .. i, lives in four rolling words (MatchRowNear, match_row_push);
//   * the candidate side — up to four windows per table — and e = x[c] of both tables are ten independent loads, one lane each
//     (match_row_lane_load: lanes 0..3 the short table's windows, 4..7 the long table's, 8 and 9 the two e), one round trip, combined
//     with shuffles (match_row_length, match_row_finish).  A window is read BYTE BY BYTE (match_row_far_window): every index lies in
//     [0, c) and c <= i < known = i + 1, whatever the block's offset in the output and however short the block.
#pragma once
#include "w3_match_plan.h"

#if defined(__clang__)
#define W3_MATCH_UNROLL _Pragma("unroll")
#else
#define W3_MATCH_UNROLL
#endif

namespace w3 {

enum { MATCH_ROW_LANES = 16, MATCH_ROW_LOAD_LANES = 10 };

// the row's context word of boundary i + 1 if byte i's low nibble is r; W_hi: the bit history after the byte's first nibble
W3_MATCH_HD uint64_t match_row_word(uint64_t W_hi, uint32_t r) { return (W_hi << 4) | (uint64_t)r; }

// the lane whose candidate word was the right one: it hands its two entries to the row and it alone stores
W3_MATCH_HD bool match_row_is_writer(uint32_t r, uint32_t byte) { return r == (byte & 15u); }

// table t (0: m bytes of context, 1: 2m) takes part at boundary i1
W3_MATCH_HD bool match_row_active(uint32_t i1, uint32_t m, uint32_t t) { return i1 >= (m << t); }

// the boundary side of the compare: w[q] = match_window's word ending at boundary - 8q.  All zero at the block start.
struct MatchRowNear { uint64_t w[4] = {0ull, 0ull, 0ull, 0ull}; };
// one more byte is known: W is the new boundary's context word
W3_MATCH_HD void match_row_push(MatchRowNear &n, uint64_t W) {
    n.w[3] = (n.w[3] << 8) | (n.w[2] >> 56);
    n.w[2] = (n.w[2] << 8) | (n.w[1] >> 56);
    n.w[1] = (n.w[1] << 8) | (n.w[0] >> 56);
    n.w[0] = W;
}
// w[idx] by selection (a run-time index into the struct would put it into scratch memory on the device)
W3_MATCH_HD uint64_t match_row_near_word(const MatchRowNear &n, uint32_t idx) { return idx == 0u ? n.w[0] : idx == 1u ? n.w[1] : idx == 2u ? n.w[2] : n.w[3]; }

// What lane r of the row fetches for boundary i1 = known with the candidates c0 (table m) and c1 (table 2m), the bytes [0, known) decoded
// (scalars, not an array: the device compiler turns a selection between two array elements back into a run-time index, i.e. scratch memory):
// lanes 0..7: the bytes of agreement (0..8) of window q = 8 (r & 3) of table r >> 2, or 8 where match_length never looks;
// lanes 8, 9: e = x[c] of table r - 8 (0 without a candidate); other lanes: 0.
// The window is match_window(blk, known, c - q) by single-byte loads through `ld` (byte index -> value): EIGHT UNCONDITIONAL loads per
// lane, so that they are in flight together (a load behind a branch of its own is waited for before the next is issued) — a byte the
// lane does not need is read from index 0, which every block with a boundary has (known >= 1), and dropped.
template <class LoadByte>
W3_MATCH_HD uint32_t match_row_lane_load(LoadByte ld, const MatchRowNear &near, uint32_t known, uint32_t c0, uint32_t c1, uint32_t r) {
    const bool win = r < 8u, el = !win && r < (uint32_t)MATCH_ROW_LOAD_LANES;
    const uint32_t ct = win ? ((r >> 2) ? c1 : c0) : el ? (r == 8u ? c0 : c1) : 0u;
    const uint32_t q = win ? 8u * (r & 3u) : 0u;
    const uint32_t limit = ct < (uint32_t)MATCH_CAP ? ct : (uint32_t)MATCH_CAP;
    const bool need_w = win && q < limit, need_e = el && ct != 0u;   // (q < limit <= ct: the window's end ct - q is at least 1)
    const uint32_t end = need_w ? ct - q : 0u;
    uint64_t W = 0ull;
    (void)known;
    W3_MATCH_UNROLL
    for (uint32_t s = 0; s < 8u; s++) {   // (s = 0 is the word's low byte, the byte right before `end`; zeros before the block start)
        const bool take = (need_w && s < end) || (need_e && s == 0u);
        const uint32_t idx = !take ? 0u : need_w ? end - 1u - s : ct;
        W3_MATCH_CHECK(idx, 1u, known);
        const uint64_t byte = ld(idx) & 0xFFu;
        W |= (take ? byte : 0ull) << (8u * s);
    }
    if (need_w) return match_equal_bytes(match_row_near_word(near, r & 3u), W);
    if (need_e) return (uint32_t)W;
    return win ? 8u : 0u;
}

// match_length from the four lanes' answers of one table
W3_MATCH_HD uint32_t match_row_length(const uint32_t eq[4], uint32_t c) {
    if (c == 0u) return 0u;
    const uint32_t limit = c < (uint32_t)MATCH_CAP ? c : (uint32_t)MATCH_CAP;
    uint32_t r = 0;
    bool open = true;   // (match_length's loop with its break, over a constant four windows: no run-time index)
    W3_MATCH_UNROLL
    for (uint32_t w = 0; w < 4u; w++) {
        if (open && 8u * w < limit) { r = 8u * w + eq[w]; open = eq[w] >= 8u; }
    }
    return r < limit ? r : limit;
}

// the choice between the tables, as match_advance ends
W3_MATCH_HD void match_row_finish(MatchState &s, uint32_t v0, uint32_t v1, uint32_t e0, uint32_t e1) {
    const bool lng = match_takes_long(v0, v1);
    const uint32_t vt = lng ? v1 : v0, et = lng ? e1 : e0;
    s.lq = vt ? match_lq(vt) : 0u;
    s.e = vt ? et : 0u;
}

}   // namespace w3
