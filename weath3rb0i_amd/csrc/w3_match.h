// w3_match.h — the key stage of the match-model leaf (W3_HIST_MATCH: OrderNEntropy(11, 3, MatchHistory(m, L))).  The
// leaf's context is a pure function of the input bytes before each position, so — DESIGN.md 3 point 1 — a parallel key stage feeds the
// time-ordered Counter kernel that exists: k_match_keys leaves the 8 keys of every byte as one uint2 in ws.keys, exactly what k_achash
// and k_huffkeys<false> leave, and the leaf then runs k_predict_small<8, true> unchanged.
//
// k_match_keys: one WAVEFRONT per block (grid-stride over the blocks), 64 consecutive byte boundaries per round (lane = boundary), the
// two candidate tables T_m and T_2m in HBM, private to the wavefront.  Per table and round:
//   * every lane reads T[h], the table's state before the round;
//   * lanes of the round with the same h are found with ballots over the hash bits (a 6-bit pre-test first: hashes of m..8 bytes rarely
//     repeat inside 64 boundaries, a block of one repeated byte being the exception); a lane's candidate is the nearest lower lane of
//     its group, else the entry read; only the highest lane of a group stores;
//   * no LDS, no atomic read-modify-write, nothing that depends on the order in which lanes' memory operations return.
// Table entries carry the wavefront's block sequence number (w3_match_plan.h: match_entry), so the tables are zeroed once per 255 blocks
// instead of once per block (2^L entries each: 8 x the bytes of a 64 KiB block at L = 16).  Entries are read and written with agent-scope
// accesses (they bypass the L1, which a store of another lane does not update), and a round's stores are waited for before the next
// round's loads are issued (k_predict_wave's rule, w3_predict_wave.h).
// The backward compare (match_length) and every other index: w3_match_plan.h, shared with the host.
#pragma once
#include "w3_match_plan.h"
#include "w3_predict_wave.h"

namespace w3 {

struct MatchKeyArgs {
    const uint8_t *in;
    uint64_t n;
    uint32_t block_size, nblocks;
    uint2 *keys;             // [n] 8 x u8 keys per byte
    uint32_t *tables;        // per resident wavefront: T_m then T_2m, 2^L u32 each
    uint32_t m, L;
};

__global__ void __launch_bounds__(64) k_match_keys(MatchKeyArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t *tbl = a.tables + ((uint64_t)blockIdx.x << (a.L + 1u));
    const uint64_t tbl_words = 2ull << a.L;
    uint32_t seq = 0;
    for (uint32_t b = blockIdx.x; b < a.nblocks; b += gridDim.x, seq++) {
        const uint64_t off = (uint64_t)b * a.block_size;
        const uint32_t len = (uint32_t)((a.n - off) < a.block_size ? (a.n - off) : a.block_size);
        const uint8_t *blk = a.in + off;
        const uint32_t tag = seq % W3_MATCH_TAGS + 1u;
        if (tag == 1u) {   // the first block of this wavefront, and every 255th after it: all entries empty
            for (uint64_t w = (uint64_t)lane * 4u; w < tbl_words; w += 256u) *reinterpret_cast<uint4 *>(tbl + w) = make_uint4(0u, 0u, 0u, 0u);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __builtin_amdgcn_s_waitcnt(0);
        }
        for (uint32_t base = 0; base < len; base += 64u) {
            const uint32_t i = base + lane;
            const bool valid = i < len;
            const uint64_t W = valid ? match_window(blk, len, i) : 0ull;
            uint32_t c[2], v[2];
#pragma unroll
            for (uint32_t t = 0; t < 2u; t++) {
                const uint32_t k = a.m << t;
                const bool act = valid && i >= k;
                const uint32_t h = act ? match_hash(W, k, a.L) : 0u;
                uint32_t *slot = tbl + ((uint64_t)t << a.L) + h;
                const uint32_t old = act ? wv_load(slot) : 0u;
                const uint64_t am = __ballot(act);
                uint64_t M = match_value<6>(h) & am;
                if (__ballot(act && (M & (M - 1ull)) != 0ull)) M = match_value<20>(h) & am;   // (L <= 20)
                const int nl = match_nearest_lower(M, lane);
                c[t] = !act ? 0u : nl >= 0 ? base + (uint32_t)nl : match_entry_pos(tag, old);
                if (act && match_is_writer(M, lane)) wv_store(slot, match_entry(tag, i));
                v[t] = act ? match_length(blk, len, i, c[t]) : 0u;
            }
            if (valid) {
                const uint32_t t = match_takes_long(v[0], v[1]) ? 1u : 0u;
                const uint32_t lq = v[t] ? match_lq(v[t]) : 0u;
                const uint32_t e = v[t] ? blk[c[t]] : 0u, x = blk[i];
                uint32_t out[2] = {0u, 0u};
#pragma unroll
                for (uint32_t j = 0; j < 8u; j++) out[j >> 2] |= match_key(lq, e, x >> (8u - j), j) << (8u * (j & 3u));
                a.keys[off + i] = make_uint2(out[0], out[1]);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the round's stores are on their way before the next round's loads
            __builtin_amdgcn_s_waitcnt(0);
        }
    }
}

}   // namespace w3
