// w3_match_plan.h — the index arithmetic of the match-model leaf (W3_HIST_MATCH, include/w3hip.h) in plain C++, usable
// from host and device (no HIP header; tests/test_match_round.py compiles it with g++): the ONE copy of the hash, the nearest-lower-lane
// rule of a 64-boundary round, the backward compare with its bounds, the length bucket and the key.  k_match_keys (w3_match.h) and the
// lane kernels (w3_generic.h, w3_cm.h) call it; tests/match_ref.py restates it in Python integers.
//
// For a block x[0..n), byte boundary i, k in (m, 2m), i >= k:
//     v      = big-endian integer of x[i-k .. i-1]
//     h_k(i) = (v * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - L)
//     c_k    = the largest i' with k <= i' < i and h_k(i') = h_k(i), or 0          (serially: c_k = T_k[h]; T_k[h] = i)
//     v_k    = the largest r <= min(CAP, c_k) with x[i-s] == x[c_k-s] for s = 1..r  (0 when c_k = 0)
//     (c, v) = (c_2m, v_2m) if v_2m > v_m else (c_m, v_m);  v == 0: no prediction;  else e = x[c], lq = bucket(v)
//     key at bit position j = (lq << 1) | bit (7-j) of e   while the j known bits of x[i] equal e's, else 0
// Nothing outside [block start, block start + known) is ever read: `known` is the block's length in the encoders and the number of
// bytes decoded so far in the decoders.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define W3_MATCH_HD __host__ __device__ __forceinline__
#else
#define W3_MATCH_HD inline
#endif
#ifndef W3_MATCH_CHECK   // tests/host/match_round.cpp: every byte index a load touches, asserted inside the block
#define W3_MATCH_CHECK(first, count, known) ((void)0)
#endif

namespace w3 {

enum { MATCH_CAP = 32, MATCH_MIN_LEN_LO = 2, MATCH_MIN_LEN_HI = 4, MATCH_LOG_LO = 8, MATCH_LOG_HI = 20 };
enum { MATCH_BITS = 11, MATCH_ALIGN = 3 };   // the leaf is OrderNEntropy(11, 3, MatchHistory(m, L))
#define W3_MATCH_MUL 0x9E3779B97F4A7C15ull

W3_MATCH_HD bool match_params_ok(uint32_t m, uint32_t L) { return m >= MATCH_MIN_LEN_LO && m <= MATCH_MIN_LEN_HI && L >= MATCH_LOG_LO && L <= MATCH_LOG_HI; }

// W: the eight bytes before boundary i as one big-endian word (x[i-1] in the low byte); k <= 8 bytes of context
W3_MATCH_HD uint32_t match_hash(uint64_t W, uint32_t k, uint32_t L) {
    const uint64_t v = k >= 8u ? W : W & ((1ull << (8u * k)) - 1ull);
    return (uint32_t)((v * W3_MATCH_MUL) >> (64u - L));
}

// bytes [end - 8, end) of the block as one big-endian word, zeros for the part before the block start.  One unaligned 8-byte load
// wherever eight bytes lie inside [0, known); byte loads in a block shorter than that.
W3_MATCH_HD uint64_t match_window(const uint8_t *blk, uint32_t known, uint32_t end) {
    uint64_t raw;
    if (end >= 8u) {
        W3_MATCH_CHECK(end - 8u, 8u, known);
        __builtin_memcpy(&raw, blk + (end - 8u), 8);
        return __builtin_bswap64(raw);
    }
    if (end == 0u) return 0ull;
    if (known >= 8u) {
        W3_MATCH_CHECK(0u, 8u, known);
        __builtin_memcpy(&raw, blk, 8);
        return __builtin_bswap64(raw) >> (8u * (8u - end));
    }
    uint64_t W = 0;
    for (uint32_t s = 0; s < end; s++) { W3_MATCH_CHECK(s, 1u, known); W = (W << 8) | blk[s]; }
    return W;
}

// bytes of agreement, from the low (most recent) end, of two such words: 0..8
W3_MATCH_HD uint32_t match_equal_bytes(uint64_t A, uint64_t B) {
    const uint64_t x = A ^ B;
    return x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
}

// v_k of candidate c at boundary i (c < i <= known): up to four windows per side, bounded by min(CAP, c)
W3_MATCH_HD uint32_t match_length(const uint8_t *blk, uint32_t known, uint32_t i, uint32_t c) {
    if (c == 0u) return 0u;
    const uint32_t limit = c < (uint32_t)MATCH_CAP ? c : (uint32_t)MATCH_CAP;
    uint32_t r = 0;
    for (uint32_t q = 0; q < limit; q += 8u) {
        const uint32_t eq = match_equal_bytes(match_window(blk, known, i - q), match_window(blk, known, c - q));
        r = q + eq;
        if (eq < 8u) break;
    }
    return r < limit ? r : limit;   // (a window's zero padding before the block start never counts: limit <= c)
}

// the long context wins only if strictly longer
W3_MATCH_HD bool match_takes_long(uint32_t v_short, uint32_t v_long) { return v_long > v_short; }

// length bucket 1..20 of v in 1..32
W3_MATCH_HD uint32_t match_lq(uint32_t v) { return v < 16u ? v : 16u + ((v - 16u) >> 2); }

// History::hash() at bit position j of a byte whose j known bits are the low bits of `part` (lq == 0: no prediction)
W3_MATCH_HD uint32_t match_key(uint32_t lq, uint32_t e, uint32_t part, uint32_t j) {
    if (lq == 0u || (part & ((1u << j) - 1u)) != (e >> (8u - j))) return 0u;
    return (lq << 1) | ((e >> (7u - j)) & 1u);
}

// ---- one round of 64 consecutive boundaries, lane = boundary: lanes that meet the same table entry ------------------------------------
// M: the lanes of the round whose hash equals this lane's (itself included), among the lanes that take part.
// The candidate of a lane is the nearest LOWER lane of its group, if there is one (else the table's state before the round) ...
W3_MATCH_HD int match_nearest_lower(uint64_t M, uint32_t lane) {
    const uint64_t lower = M & ((1ull << lane) - 1ull);
    return lower ? 63 - (int)__builtin_clzll(lower) : -1;
}
// ... and only the highest lane of a group stores.
W3_MATCH_HD bool match_is_writer(uint64_t M, uint32_t lane) { return (M >> lane) >> 1 == 0ull; }

// a table entry of the wavefront kernel: the boundary tagged with the wavefront's block sequence (1..255), so that an entry of an
// earlier block never passes for a candidate; boundaries are below 2^24 (the two-phase path's block size limit)
#define W3_MATCH_TAGS 255u
W3_MATCH_HD uint32_t match_entry(uint32_t tag, uint32_t i) { return (tag << 24) | i; }
W3_MATCH_HD uint32_t match_entry_pos(uint32_t tag, uint32_t entry) { return (entry >> 24) == tag ? entry & 0xFFFFFFu : 0u; }

// ---- the serial form (lane-per-block kernels; the host's truth of the round form) -----------------------------------------------------
struct MatchState { uint32_t e = 0u, lq = 0u; };

// boundary i of a block whose bytes [0, i) are known (i >= 1): look both contexts up, record i, choose.  T: T_m then T_2m, 2^L u32 each,
// zero at the block start.
W3_MATCH_HD void match_advance(MatchState &s, uint32_t *T, uint32_t m, uint32_t L, const uint8_t *blk, uint32_t known, uint32_t i) {
    const uint64_t W = match_window(blk, known, i);
    uint32_t c[2] = {0u, 0u}, v[2] = {0u, 0u};
    for (uint32_t t = 0; t < 2u; t++) {
        const uint32_t k = m << t;
        if (i < k) continue;
        uint32_t *slot = T + ((uint64_t)t << L) + match_hash(W, k, L);
        c[t] = *slot;
        *slot = i;
        v[t] = match_length(blk, known, i, c[t]);
    }
    const uint32_t t = match_takes_long(v[0], v[1]) ? 1u : 0u;
    s.lq = v[t] ? match_lq(v[t]) : 0u;
    if (v[t]) { W3_MATCH_CHECK(c[t], 1u, known); s.e = blk[c[t]]; } else s.e = 0u;
}

}   // namespace w3
