// w3_export_entropy.h — the parallel context statistics export (w3_export.h) for OrderNEntropy leaves (w3_export_entropy_device / _staged):
// the Counter table of ONE adaptive OrderNEntropy(bits, align, ACHistory | HuffHistory) leaf after it has seen the input as one stream.
// In the form of w3_export.h: the arithmetic is plain C++ over a `Wave` type, the kernels are below it (tests/test_export_entropy_cpu.py
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
//       it crosses epoch cuts freely and at the PIECE's start comes from carry8, the 8 stream bytes before the piece.
//   HuffHistory keys  k_expk_huffkeys: one thread per byte walks back at most W3_HUFF_WALK bytes (k_huffkeys' bounded walk) until 32 bits
//       are covered.  A walk that reaches the piece's first byte takes the rest from the piece's seed (compressed_bits there; 0 at the
//       stream's start).  A walk that ends uncovered with bytes left (a run of zero-length codes) flags the epoch; k_expk_huff_fix
//       then redoes the epoch's keys with the reference's own recurrence from the epoch's seed: the compressed_bits the previous epoch's
//       fix-up ended with when that ran, else a walk back from the epoch's first byte — which ends within W3_HUFF_WALK + 1 bytes or at
//       the piece's start, because no position of an unflagged epoch was left uncovered.  All in stream order on the device.
//   keyed count  k_expk_count_lds / k_expk_count: k_ctx_count's two forms over K, 16 bytes (four steps) per lane and load.
//   apply  k_ctx_apply, unchanged.
//   keyed replay  k_expk_replay: exp_replay's scheme over rows of 256 steps (lane l: steps 4 l .. 4 l + 3), W3_EXPK_REPLAY_ROWS rows
//       counted together, walked row by row only where a count can reach 65535; a row holds at most one halving of a context.
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

// A piece of the stream on the device: [p, p + n) is stream [abs0, abs0 + n); carry8 = the eight stream bytes before it, big-endian (the
// last one in bits 0 .. 7; zeros where the stream has not begun); seed = HuffHistory's compressed_bits at its first byte
struct ExpKeyPiece {
    const uint8_t *p;
    uint64_t n, abs0, carry8;
    uint32_t seed;
};

// the key of a step: `hash` = History::hash() before it, absbit = its bit index in the stream
W3_HD uint32_t expk_key(const ExpModel &m, uint32_t hash, uint64_t absbit, uint32_t bit) {
    const uint32_t hmask = (uint32_t)((1ull << (m.bits - m.align)) - 1ull), amask = (1u << m.align) - 1u;
    const uint32_t ctx = absbit ? ((hash & hmask) << m.align) | ((uint32_t)absbit & amask) : 0u;   // (ordern_entropy.rs:19: ctx starts at 0)
    return ctx | (bit << 31);
}

// the 64 stream bits before byte i of the piece (0 <= i <= n), newest at bit 0: what the next piece's carry8 is for i = n
W3_HHD uint64_t expk_window(const ExpKeyPiece &pc, uint64_t i) {
    if (i >= 8u) {
        uint64_t raw;
        __builtin_memcpy(&raw, pc.p + (i - 8u), 8);
        return __builtin_bswap64(raw);
    }
    uint64_t h = pc.carry8;
    for (uint32_t k = 0; k < 7u; k++)
        if (k < i) h = (h << 8) | pc.p[k];
    return h;
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
W3_HD bool expk_huff_byte(const ExpKeyPiece &pc, uint64_t e0, uint64_t g, const ExpModel &m, const Code *code, const Len *len, const Code *rcode,
                          const Len *rlen, uint32_t (&k)[8]) {
    const uint64_t i = e0 + g;
    const ExpHuffCb r = expk_huff_back(pc.p, i, 0u, W3_HUFF_WALK, code, len);
    const bool open = r.have < 32u && r.at != 0u;
    expk_huff_keys(m, expk_huff_join(r, pc.seed), pc.p[i], pc.abs0 + i, rcode, rlen, k);
    return !open;
}

// compressed_bits at the first byte of the epoch at e0: `chained` = the previous epoch of this piece was redone and ended with chain_cb
template <class Code, class Len>
W3_HD uint32_t expk_huff_epoch_seed(const ExpKeyPiece &pc, uint64_t e0, bool chained, uint32_t chain_cb, const Code *code, const Len *len) {
    if (chained) return chain_cb;
    return expk_huff_join(expk_huff_back(pc.p, e0, 0u, ~0ull, code, len), pc.seed);
}

// the epoch's keys by the recurrence (huff_history.rs:60-66) from compressed_bits at its first byte; returns compressed_bits behind it
template <class Code, class Len>
W3_HD uint32_t expk_huff_redo(const ExpKeyPiece &pc, uint64_t e0, uint64_t len, const ExpModel &m, uint32_t cb, const Code *code, const Len *clen,
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

// four consecutive steps of K as a lane loads them (K is 16-byte aligned and an epoch has a multiple of eight steps)
struct alignas(16) ExpK4 { uint32_t k[4]; };
W3_HD ExpK4 expk_load4(const uint32_t *K, uint64_t steps, uint64_t at) {
    if (at < steps) return *reinterpret_cast<const ExpK4 *>(K + at);
    return ExpK4{{W3_EXPK_NONE, W3_EXPK_NONE, W3_EXPK_NONE, W3_EXPK_NONE}};
}
W3_HHD uint64_t expk_rows(uint64_t steps) { return (steps + 255u) >> 8; }

// count: lane `lane` of wave gw (of nw waves) takes the rows gw, gw + nw, ..., W3_EXPK_COUNT_ROWS of them in flight: add(ctx, bit) per step
template <class Add>
W3_HD void expk_count_wave_lane(const uint32_t *K, uint64_t steps, uint32_t lane, uint64_t gw, uint64_t nw, Add add) {
    const uint64_t rows = expk_rows(steps);
    for (uint64_t r = gw; r < rows; r += nw * W3_EXPK_COUNT_ROWS) {
        ExpK4 x[W3_EXPK_COUNT_ROWS];
        W3_EXP_UNROLL
        for (uint32_t u = 0; u < W3_EXPK_COUNT_ROWS; u++) x[u] = expk_load4(K, steps, (r + u * nw) * 256u + lane * 4u);   // the loads first
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

// replay, one row: (c0, c1) is context `target`'s state at the row's first step and on return behind its last.  Returns the halvings.
template <class WV>
W3_HD uint32_t expk_replay_row(WV &wv, const uint32_t *K, uint64_t steps, uint64_t row, uint32_t target, uint32_t &c0, uint32_t &c1) {
    typename WV::template Vec<uint32_t> mz, mo, o0, o1, p0, p1, hit;   // mz / mo: the lane's matching steps with bit 0 / bit 1
    wv.each([&](uint32_t l) {
        const ExpK4 x = expk_load4(K, steps, row * 256u + l * 4u);
        uint32_t z = 0, o = 0;
        W3_EXP_UNROLL
        for (uint32_t q = 0; q < 4u; q++) {
            z |= (uint32_t)(x.k[q] == target) << q;
            o |= (uint32_t)(x.k[q] == (target | W3_EXPK_BIT)) << q;
        }
        mz[l] = z; mo[l] = o;
        o0[l] = p0[l] = prep_popc32(z);
        o1[l] = p1[l] = prep_popc32(o);
    });
    wv.incl_scan(p0);
    wv.incl_scan(p1);
    const uint32_t a0 = c0, a1 = c1;
    wv.each([&](uint32_t l) { hit[l] = (a0 + p0[l] >= W3_STAT_LIMIT || a1 + p1[l] >= W3_STAT_LIMIT) ? 1u : 0u; });
    const uint64_t lanes = wv.ballot(hit);
    const uint32_t t0 = wv.get(p0, 63u), t1 = wv.get(p1, 63u);
    if (!lanes) { c0 += t0; c1 += t1; return 0u; }
    const uint32_t g = prep_ctz64(lanes);   // the lane whose four steps hold the halving
    const uint32_t g0 = wv.get(p0, g), g1 = wv.get(p1, g);
    c0 += g0 - wv.get(o0, g);
    c1 += g1 - wv.get(o1, g);
    const uint32_t z = wv.get(mz, g), o = wv.get(mo, g);
    uint32_t halvings = 0;
    for (uint32_t q = 0; q < 4u; q++)   // that lane's matches in order (every lane walks the same values)
        if (((z | o) >> q) & 1u) halvings += exp_counter_update(c0, c1, (o >> q) & 1u);
    c0 += t0 - g0;   // the rest of the row: 256 steps hold at most one halving of a context
    c1 += t1 - g1;
    return halvings;
}

// lane l's visits of `target` by bit value in the rows r .. r + W3_EXPK_REPLAY_ROWS - 1 (rows behind the epoch's end are empty): the loads first
W3_HD void expk_block_count(const uint32_t *K, uint64_t steps, uint64_t r, uint32_t l, uint32_t target, uint32_t &n0, uint32_t &n1) {
    ExpK4 x[W3_EXPK_REPLAY_ROWS];
    W3_EXP_UNROLL
    for (uint32_t u = 0; u < W3_EXPK_REPLAY_ROWS; u++) x[u] = expk_load4(K, steps, (r + u) * 256u + l * 4u);
    W3_EXP_UNROLL
    for (uint32_t u = 0; u < W3_EXPK_REPLAY_ROWS; u++) {
        W3_EXP_UNROLL
        for (uint32_t q = 0; q < 4u; q++) {
            n0 += x[u].k[q] == target ? 1u : 0u;
            n1 += x[u].k[q] == (target | W3_EXPK_BIT) ? 1u : 0u;
        }
    }
}

// replay of context `target` over the epoch's keys: s = its state before the epoch, on return behind it.  Returns the halvings.
template <class WV>
W3_HD uint32_t expk_replay(WV &wv, const uint32_t *K, uint64_t steps, uint32_t target, uint32_t &s) {
    const uint64_t rows = expk_rows(steps);
    uint32_t c0 = s & 0xFFFFu, c1 = s >> 16, halvings = 0;
    typename WV::template Vec<uint32_t> q0, q1;
    for (uint64_t r = 0; r < rows; r += W3_EXPK_REPLAY_ROWS) {
        wv.each([&](uint32_t l) {
            uint32_t n0 = 0, n1 = 0;
            expk_block_count(K, steps, r, l, target, n0, n1);
            q0[l] = n0; q1[l] = n1;
        });
        wv.incl_scan(q0);
        wv.incl_scan(q1);
        const uint32_t t0 = wv.get(q0, 63u), t1 = wv.get(q1, 63u);
        if (c0 + t0 < W3_STAT_LIMIT && c1 + t1 < W3_STAT_LIMIT) { c0 += t0; c1 += t1; continue; }
        for (uint64_t k = r; k < r + W3_EXPK_REPLAY_ROWS && k < rows; k++) halvings += expk_replay_row(wv, K, steps, k, target, c0, c1);
    }
    s = c0 | (c1 << 16);
    return halvings;
}

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
    ExpKeyPiece pc; uint64_t e0, len; ExpModel m; uint32_t max_bits; uint16_t table[8];
    const uint4 *lut;   // [65536][8] (k_achash_lut)
    uint32_t *K;
};

// ACHistory keys: one thread per step of the epoch (a grid-stride loop: a dispatch counts its work-items in 32 bits)
__global__ void __launch_bounds__(256) k_expk_ackeys(ExpAcArgs a) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.len * 8u; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = a.e0 + (g >> 3);
        const uint32_t j = (uint32_t)g & 7u, c0 = a.pc.p[i];
        const uint64_t hist = (expk_window(a.pc, i) << j) | (uint64_t)(c0 >> (8u - j));   // the last 64 bits before bit j of byte i, newest at bit 0
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
    ExpKeyPiece pc; uint64_t e0, len; ExpModel m;
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

// keyed count in the workgroup's LDS table (k_ctx_count_lds over K)
template <uint32_t REP>
__global__ void __launch_bounds__(256) k_expk_count_lds(const uint32_t *K, uint64_t steps, ExpModel m, exp_u64 *D, uint32_t *stats) {
    extern __shared__ uint32_t exp_tab[];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nctx = 1u << m.bits;
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[W3_EXP_ST_LISTED] = 0u;
    for (uint32_t k = threadIdx.x; k < 2u * nctx * REP; k += 256u) exp_tab[k] = 0u;
    __syncthreads();
    uint32_t *mine = exp_tab + (lane & (REP - 1u));
    expk_count_wave_lane(K, steps, lane, (uint64_t)blockIdx.x * 4u + wv, (uint64_t)gridDim.x * 4u, [&](uint32_t ctx, uint32_t bit) {
        (void)__hip_atomic_fetch_add(&mine[(2u * ctx + bit) * REP], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    });
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < nctx; c += 256u) {
        uint32_t d0 = 0, d1 = 0;
        for (uint32_t r = 0; r < REP; r++) { d0 += exp_tab[2u * c * REP + r]; d1 += exp_tab[(2u * c + 1u) * REP + r]; }
        if (d0 | d1) (void)__hip_atomic_fetch_add(&D[c], (exp_u64)d0 | ((exp_u64)d1 << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// keyed count with one 64-bit device add per step
__global__ void __launch_bounds__(256) k_expk_count(const uint32_t *K, uint64_t steps, exp_u64 *D, uint32_t *stats) {
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[W3_EXP_ST_LISTED] = 0u;
    expk_count_wave_lane(K, steps, threadIdx.x & 63u, (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6), (uint64_t)gridDim.x * 4u,
                         [&](uint32_t ctx, uint32_t bit) {
                             (void)__hip_atomic_fetch_add(&D[ctx], bit ? 1ull << 32 : 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                         });
}

// keyed replay: a wavefront per listed context, as k_ctx_replay
__global__ void __launch_bounds__(64) k_expk_replay(const uint32_t *K, uint64_t steps, uint32_t *S, const uint32_t *list, uint32_t cap, uint32_t *stats) {
    WaveDev wv{threadIdx.x & 63u};
    const uint32_t listed = stats[W3_EXP_ST_LISTED], count = listed < cap ? listed : cap;
    uint32_t halvings = 0;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t c = list[i];
        uint32_t s = S[c];
        halvings += expk_replay(wv, K, steps, c, s);
        if (wv.lane == 0) S[c] = s;
    }
    if (wv.lane == 0) {
        if (halvings) (void)__hip_atomic_fetch_add(&stats[W3_EXP_ST_HALVINGS], halvings, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (blockIdx.x == 0) stats[W3_EXP_ST_REPLAYS] += count;   // (one writer per launch, launches in stream order)
    }
}

}  // namespace w3
#endif
