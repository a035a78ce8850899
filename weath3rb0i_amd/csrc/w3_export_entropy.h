// w3_export_entropy.h — what OrderNEntropy leaves add to the parallel context statistics export (w3_export.h; w3_export_entropy_device /
// _staged): the Counter table of ONE adaptive OrderNEntropy(bits, align, ACHistory | HuffHistory) leaf after it has seen the input as one
// stream.  This file holds the KEY STAGE and the KEYED STEP SOURCE and nothing else: count, apply and replay are w3_export.h's, written
// once over a source.  In the form of w3_export.h: the arithmetic is plain C++, the kernels are below it (tests/test_export_entropy_cpu.py
// compiles the upper part with g++ and drives it through tests/host/export_entropy_lanes.cpp).
//
// WHY IT IS NOT SERIAL EITHER.  OrderNEntropy's context is (History::hash() & mask) << align | bit index mod 2^align
// (ordern_entropy.rs:36-45), and both entropy histories hash a pure function of the input:
//   ACHistory::hash (ac_history.rs:28-46) starts a fresh coder on every call and codes at most the last 64 history bits under pos & 7:
//       a function of the 8 bytes before the step's byte, the partial byte and the bit position.
//   HuffHistory::hash (huff_history.rs:60-72) reads compressed_bits, the fold cb = cb << len | code over all bytes before the step's
//       byte, cut to 32 bits: a function of the trailing bytes whose code lengths sum to 32.
// w3_export.h's argument about the Counters (order matters only where one halves) carries over unchanged.
//
// THE ALGORITHM.  Per epoch of E bytes a KEY STAGE fills K with one uint32 per step, ctx | bit << 31 (ctx < 2^28: the finished table
// index); count and replay then read only K.  Step 0 of the STREAM has ctx = 0 (ordern_entropy.rs:19) whatever the empty history hashes
// to.  K takes 32 E bytes: keyed epochs are clamped to W3_EXPK_EPOCH_MAX.
//   ACHistory keys  k_expk_ackeys: one thread per step; the coder state after the 16 most recent history bits comes from k_achash_lut's
//       table, the rest is coded from there (ac_history_hash_steps), as k_achash32 does.  The window is the 64 stream bits before the step:
//       it crosses epoch cuts freely and at the PIECE's start comes from the piece's carry, the 8 stream bytes before it.
//   HuffHistory keys  k_expk_huffkeys: one thread per byte walks back at most W3_HUFF_WALK bytes (k_huffkeys' bounded walk) until 32 bits
//       are covered.  A walk that reaches the piece's first byte takes the rest from the piece's seed (compressed_bits there; 0 at the
//       stream's start).  A walk that ends uncovered with bytes left (a run of zero-length codes) flags the epoch; k_expk_huff_fix
//       then redoes the epoch's keys with the reference's own recurrence from the epoch's seed: the compressed_bits the previous epoch's
//       fix-up ended with when that ran, else a walk back from the epoch's first byte — which ends within W3_HUFF_WALK + 1 bytes or at
//       the piece's start, because no position of an unflagged epoch was left uncovered.  All in stream order on the device.
//   keyed source  ExpKeySrc: K as rows of 256 steps (lane l: steps 4 l .. 4 l + 3, one 16-byte load), W3_EXPK_COUNT_ROWS rows of a wave
//       in flight in the count (k_exp_count_lds<ExpKeySrc, REP> / k_exp_count<ExpKeySrc>), W3_EXPK_REPLAY_ROWS rows counted together in the
//       replay (k_exp_replay<ExpKeySrc>) and walked row by row only where a count can reach 65535; a row holds at most one halving of a
//       context.  k_ctx_apply does not see the source.
#pragma once
#include "w3_export.h"

namespace w3 {

#ifndef W3_HUFF_WALK
#define W3_HUFF_WALK 40u               // (w3_predict.h's, for the host build of this file)
#endif
#define W3_EXPK_EPOCH_MAX (1u << 24)   // bytes per keyed epoch at the most: 512 MiB of keys
#ifndef W3_EXPK_EPOCH_DEFAULT
#define W3_EXPK_EPOCH_DEFAULT (4u << 20)   // bytes per keyed epoch (W3_OPT_EXPORT_EPOCH = 0): the smallest median of 1, 4, 16 MiB for init_model() at 1e9 B, DESIGN.md 3.10
#endif
#define W3_EXPK_BIT 0x80000000u        // the step's bit in its key
#define W3_EXPK_NONE 0x7FFFFFFFu       // what a load behind the epoch's last step gives: no context (ctx < 2^28)
#define W3_EXPK_COUNT_ROWS 4u          // rows a wave of the count has in flight
#ifndef W3_EXPK_REPLAY_ROWS
#define W3_EXPK_REPLAY_ROWS 32u        // rows of a replay whose loads are issued together and whose counts are summed at once (8: 1.5 x the replay's time)
#endif
static_assert(W3_EXPK_EPOCH_MAX % 1024u == 0 && W3_EXPK_EPOCH_MAX <= W3_EXP_EPOCH_MAX, "a keyed epoch: whole KiB, an epoch of w3_export.h");
static_assert(W3_EXPK_EPOCH_DEFAULT % 1024u == 0 && W3_EXPK_EPOCH_DEFAULT <= W3_EXPK_EPOCH_MAX, "the keyed default: whole KiB, at most the clamp");

// the key of a step: `hash` = History::hash() before it, absbit = its bit index in the stream
W3_HD uint32_t expk_key(const ExpModel &m, uint32_t hash, uint64_t absbit, uint32_t bit) {
    const uint32_t hmask = (uint32_t)((1ull << (m.bits - m.align)) - 1ull), amask = (1u << m.align) - 1u;
    const uint32_t ctx = absbit ? ((hash & hmask) << m.align) | ((uint32_t)absbit & amask) : 0u;   // (ordern_entropy.rs:19: ctx starts at 0)
    return ctx | (bit << 31);
}

// HuffHistory: the codes of the bytes [at, i) of the piece, newest lowest: `have` bits of compressed_bits before byte i
struct ExpHuffCb {
    uint32_t cb, have;
    uint64_t at;
};
// walk back from byte i over at most `max` bytes, not below byte `lo`, until 32 bits are covered (code lengths <= 16: parse_spec)
template <class Code, class Len>
W3_HHD ExpHuffCb expk_huff_back(const uint8_t *p, uint64_t i, uint64_t lo, uint64_t max, const Code *code, const Len *len) {
    ExpHuffCb r = {0u, 0u, i};
    while (r.at > lo && r.have < 32u && i - r.at < max) {
        const uint32_t byte = p[r.at - 1u];
        r.cb |= (uint32_t)code[byte] << r.have;
        r.have += len[byte];
        r.at--;
    }
    return r;
}
// ... completed by compressed_bits at byte r.at
W3_HHD uint32_t expk_huff_join(const ExpHuffCb &r, uint32_t seed) { return r.have < 32u ? r.cb | (seed << r.have) : r.cb; }

// compressed_bits at stream byte o0 of the host's whole input, given it at byte `prev` <= o0 (the piece before's first byte): the
// staged form's seed chain, a walk back through one piece at the most
template <class Code, class Len>
W3_HHD uint32_t expk_huff_piece_seed(const uint8_t *in, uint64_t o0, uint64_t prev, uint32_t seed_prev, const Code *code, const Len *len) {
    return expk_huff_join(expk_huff_back(in, o0, prev, ~0ull, code, len), seed_prev);
}

// the 8 keys of byte c0 (stream byte absbyte) given compressed_bits before it (huff_history.rs:67-71)
template <class Code, class Len>
W3_HD void expk_huff_keys(const ExpModel &m, uint32_t cb, uint32_t c0, uint64_t absbyte, const Code *rcode, const Len *rlen, uint32_t (&k)[8]) {
    W3_EXP_UNROLL
    for (uint32_t j = 0; j < 8u; j++) {
        const uint32_t rem = (1u << j) | (c0 >> (8u - j));
        k[j] = expk_key(m, (cb << rlen[rem]) | rcode[rem], absbyte * 8u + j, (c0 >> (7u - j)) & 1u);
    }
}

// the keys of byte g of the epoch [e0, e0 + len) by the bounded walk.  False: the walk ended uncovered with bytes left (k is not valid)
template <class Code, class Len>
W3_HD bool expk_huff_byte(const ExpPiece &pc, uint64_t e0, uint64_t g, const ExpModel &m, const Code *code, const Len *len, const Code *rcode,
                          const Len *rlen, uint32_t (&k)[8]) {
    const uint64_t i = e0 + g;
    const ExpHuffCb r = expk_huff_back(pc.p, i, 0u, W3_HUFF_WALK, code, len);
    const bool open = r.have < 32u && r.at != 0u;
    expk_huff_keys(m, expk_huff_join(r, pc.seed), pc.p[i], pc.abs0 + i, rcode, rlen, k);
    return !open;
}

// compressed_bits at the first byte of the epoch at e0: `chained` = the previous epoch of this piece was redone and ended with chain_cb
template <class Code, class Len>
W3_HD uint32_t expk_huff_epoch_seed(const ExpPiece &pc, uint64_t e0, bool chained, uint32_t chain_cb, const Code *code, const Len *len) {
    if (chained) return chain_cb;
    return expk_huff_join(expk_huff_back(pc.p, e0, 0u, ~0ull, code, len), pc.seed);
}

// the epoch's keys by the recurrence (huff_history.rs:60-66) from compressed_bits at its first byte; returns compressed_bits behind it
template <class Code, class Len>
W3_HD uint32_t expk_huff_redo(const ExpPiece &pc, uint64_t e0, uint64_t len, const ExpModel &m, uint32_t cb, const Code *code, const Len *clen,
                              const Code *rcode, const Len *rlen, uint32_t *K) {
    for (uint64_t g = 0; g < len; g++) {
        const uint32_t c0 = pc.p[e0 + g];
        uint32_t k[8];
        expk_huff_keys(m, cb, c0, pc.abs0 + e0 + g, rcode, rlen, k);
        for (uint32_t j = 0; j < 8u; j++) K[8u * g + j] = k[j];
        cb = (cb << clen[c0]) | code[c0];
    }
    return cb;
}

// ---------------------------------------------------------------------------
// The keyed source (w3_export.h's contract): the epoch's keys K[0 .. steps).  Rows of 256 steps, lane l: steps 4 l .. 4 l + 3 of a row.
// ---------------------------------------------------------------------------
struct ExpKeySrc {
    const uint32_t *K;   // 16-byte aligned
    uint64_t steps;      // a multiple of eight
    typedef uint32_t Mask;
    static constexpr uint32_t MASK_WORDS = 1u, BLOCK_ROWS = W3_EXPK_REPLAY_ROWS;
};
// four consecutive steps of K as a lane loads them
struct alignas(16) ExpK4 { uint32_t k[4]; };
W3_HD ExpK4 expk_load4(const ExpKeySrc &s, uint64_t at) {
    if (at < s.steps) return *reinterpret_cast<const ExpK4 *>(s.K + at);
    return ExpK4{{W3_EXPK_NONE, W3_EXPK_NONE, W3_EXPK_NONE, W3_EXPK_NONE}};
}
W3_HHD uint64_t exp_rows(const ExpKeySrc &s) { return (s.steps + 255u) >> 8; }

// W3_EXPK_COUNT_ROWS rows of a wave in flight
template <class Add>
W3_HD void exp_count_wave_lane(const ExpKeySrc &s, uint32_t lane, uint64_t gw, uint64_t nw, Add add) {
    const uint64_t rows = exp_rows(s);
    for (uint64_t r = gw; r < rows; r += nw * W3_EXPK_COUNT_ROWS) {
        ExpK4 x[W3_EXPK_COUNT_ROWS];
        W3_EXP_UNROLL
        for (uint32_t u = 0; u < W3_EXPK_COUNT_ROWS; u++) x[u] = expk_load4(s, (r + u * nw) * 256u + lane * 4u);   // the loads first
        W3_EXP_UNROLL
        for (uint32_t u = 0; u < W3_EXPK_COUNT_ROWS; u++) {
            W3_EXP_UNROLL
            for (uint32_t q = 0; q < 4u; q++) {
                const uint32_t k = x[u].k[q];
                if ((k & ~W3_EXPK_BIT) != W3_EXPK_NONE) add(k & ~W3_EXPK_BIT, k >> 31);
            }
        }
    }
}

W3_HD void exp_row_masks(const ExpKeySrc &s, uint64_t row, uint32_t l, uint32_t target, uint32_t (&z)[1], uint32_t (&o)[1]) {
    const ExpK4 x = expk_load4(s, row * 256u + l * 4u);
    z[0] = o[0] = 0u;
    W3_EXP_UNROLL
    for (uint32_t q = 0; q < 4u; q++) {
        z[0] |= (uint32_t)(x.k[q] == target) << q;
        o[0] |= (uint32_t)(x.k[q] == (target | W3_EXPK_BIT)) << q;
    }
}

W3_HD void exp_block_count(const ExpKeySrc &s, uint64_t r, uint32_t l, uint32_t target, uint32_t &n0, uint32_t &n1) {
    ExpK4 x[W3_EXPK_REPLAY_ROWS];
    W3_EXP_UNROLL
    for (uint32_t u = 0; u < W3_EXPK_REPLAY_ROWS; u++) x[u] = expk_load4(s, (r + u) * 256u + l * 4u);
    W3_EXP_UNROLL
    for (uint32_t u = 0; u < W3_EXPK_REPLAY_ROWS; u++) {
        W3_EXP_UNROLL
        for (uint32_t q = 0; q < 4u; q++) {
            n0 += x[u].k[q] == target ? 1u : 0u;
            n1 += x[u].k[q] == (target | W3_EXPK_BIT) ? 1u : 0u;
        }
    }
}

#ifndef __HIPCC__
// HOST BUILDS ONLY, and only until the commit before this one is no longer tested against (see the end of w3_export.h's upper part): what
// tests/host/export_entropy_lanes.cpp as it stood there drives this header through.  The library never sees these.
struct ExpKeyPiece {
    const uint8_t *p;
    uint64_t n, abs0, carry8;
    uint32_t seed;
    operator ExpPiece() const { return ExpPiece{p, n, abs0, carry8, seed}; }
};
W3_HD uint64_t expk_window(const ExpPiece &pc, uint64_t i) { return exp_window(pc, i); }
template <class Add>
W3_HD void expk_count_wave_lane(const uint32_t *K, uint64_t steps, uint32_t lane, uint64_t gw, uint64_t nw, Add add) {
    exp_count_wave_lane(ExpKeySrc{K, steps}, lane, gw, nw, add);
}
template <class WV>
W3_HD uint32_t expk_replay(WV &wv, const uint32_t *K, uint64_t steps, uint32_t target, uint32_t &s) { return exp_replay(wv, ExpKeySrc{K, steps}, target, s); }
#endif

// words of the Huffman key stage's state on the device
#define W3_EXPK_HS_FLAG 0u      // != 0: a walk of the current epoch ended uncovered (k_expk_huffkeys sets, k_expk_huff_fix clears)
#define W3_EXPK_HS_CHAINED 1u   // != 0: the previous epoch of this piece was redone ...
#define W3_EXPK_HS_CB 2u        // ... and ended with this compressed_bits
#define W3_EXPK_HS_FIXED 3u     // epochs redone
#define W3_EXPK_HS_WORDS 4u

}  // namespace w3

#ifdef __HIPCC__
namespace w3 {

struct ExpAcArgs {
    ExpPiece pc; uint64_t e0, len; ExpModel m; uint32_t max_bits; uint16_t table[8];
    const uint4 *lut;   // [65536][8] (k_achash_lut)
    uint32_t *K;
};

// ACHistory keys: one thread per step of the epoch (a grid-stride loop: a dispatch counts its work-items in 32 bits)
__global__ void __launch_bounds__(256) k_expk_ackeys(ExpAcArgs a) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.len * 8u; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = a.e0 + (g >> 3);
        const uint32_t j = (uint32_t)g & 7u, c0 = a.pc.p[i];
        const uint64_t hist = (exp_window(a.pc, i) << j) | (uint64_t)(c0 >> (8u - j));   // the last 64 bits before bit j of byte i, newest at bit 0
        uint32_t p32t[8], rot[8];
#pragma unroll
        for (int k = 0; k < 8; k++) p32t[k] = a.table[k] ? ((uint32_t)a.table[k] << 16) : 1u;   // lerp operand, arithmetic_coder.rs:111
#pragma unroll
        for (int r = 0; r < 8; r++) {   // the r-th coded history bit uses table[(j - 1 - r) & 7] (stationary.rs:54-57)
            const uint32_t k = (j + 7u - (uint32_t)r) & 7u;
            rot[r] = k == 0 ? p32t[0] : k == 1 ? p32t[1] : k == 2 ? p32t[2] : k == 3 ? p32t[3] : k == 4 ? p32t[4] : k == 5 ? p32t[5] : k == 6 ? p32t[6] : p32t[7];
        }
        const uint4 sv = a.lut[((uint32_t)hist & ((1u << W3_ACHASH_LUT_BITS) - 1u)) * 8u + j];
        ACHashState st; st.x1 = sv.x; st.x2 = sv.y; st.hash = sv.z; st.meta = sv.w;
        st = ac_history_hash_steps(hist, a.max_bits, rot, st, W3_ACHASH_LUT_BITS, 64);
        a.K[g] = expk_key(a.m, ac_hash_finish(st, a.max_bits), (a.pc.abs0 + i) * 8u + j, (c0 >> (7u - j)) & 1u);
    }
}

struct ExpHuffArgs {
    ExpPiece pc; uint64_t e0, len; ExpModel m;
    const w3_huff_table *tb;
    uint32_t *K, *hs;   // hs: W3_EXPK_HS_*
};

// HuffHistory keys: one thread per byte of the epoch, two 16-byte stores
__global__ void __launch_bounds__(256) k_expk_huffkeys(ExpHuffArgs a) {
    __shared__ uint16_t s_code[256], s_rcode[256];
    __shared__ uint8_t s_len[256], s_rlen[256];
    s_code[threadIdx.x] = a.tb->code[threadIdx.x]; s_len[threadIdx.x] = a.tb->len[threadIdx.x];
    s_rcode[threadIdx.x] = a.tb->rem_code[threadIdx.x]; s_rlen[threadIdx.x] = a.tb->rem_len[threadIdx.x];
    __syncthreads();
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.len; g += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t k[8];
        if (!expk_huff_byte(a.pc, a.e0, g, a.m, s_code, s_len, s_rcode, s_rlen, k)) a.hs[W3_EXPK_HS_FLAG] = 1u;   // (benign race: every writer stores 1)
        uint4 *dst = reinterpret_cast<uint4 *>(a.K + g * 8u);
        dst[0] = make_uint4(k[0], k[1], k[2], k[3]);
        dst[1] = make_uint4(k[4], k[5], k[6], k[7]);
    }
}

// one lane, behind k_expk_huffkeys in stream order: a flagged epoch's keys again by the recurrence; the chain for the next epoch
__global__ void __launch_bounds__(64) k_expk_huff_fix(ExpHuffArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t flagged = a.hs[W3_EXPK_HS_FLAG];
    if (flagged) {
        const uint32_t seed = expk_huff_epoch_seed(a.pc, a.e0, a.hs[W3_EXPK_HS_CHAINED] != 0u, a.hs[W3_EXPK_HS_CB], a.tb->code, a.tb->len);
        a.hs[W3_EXPK_HS_CB] = expk_huff_redo(a.pc, a.e0, a.len, a.m, seed, a.tb->code, a.tb->len, a.tb->rem_code, a.tb->rem_len, a.K);
        a.hs[W3_EXPK_HS_FIXED] += 1u;
    }
    a.hs[W3_EXPK_HS_CHAINED] = flagged;
    a.hs[W3_EXPK_HS_FLAG] = 0u;
}

}  // namespace w3
#endif
