// w3_aoh.h — "AC over Huffman", the reference's best-ratio research driver (bin/ac-over-huffman/main.rs:69-89): every input byte is
// replaced by its canonical Huffman code (package_merge + canonical, entropy_coding/package_merge.rs), the code's bits go MSB first
// ((code >> i) & 1, i = len-1 .. 0, :80-82) through the usual step  p = model.predict(); model.update(bit); ac.encode(bit, p)  (:81-84)
// with model = OrderN::new(ctx_bits, 0) (:71), then ac.flush (:87).  The context is the last ctx_bits bits of the HUFFMAN bit string: it
// runs across symbol boundaries.  A block's number of coded bits L_b = sum of len[byte] differs from block to block and is not a multiple
// of 8 — which is why none of the 8-steps-per-byte kernels can express this coder.
//
// One fused kernel, one lane per block (the form of k_sweep_ordern / k_generic), in three modes: the counting sink (ACStats; lanes =
// configurations x blocks), encode (Encoder into stripes, then w3_pack.h) and decode (Decoder, the code walked bit by bit).  The code
// table and the decode tables of the wavefront's configuration sit in LDS, copied there from device memory by the whole wavefront.
//
// The two-phase form of encode and of the counting sink (W3_PATH_TWOPHASE; the layout and the bit-string helpers are w3_aoh_plan.h's):
//   k_aoh_pack     a wavefront per block writes the block's Huffman bit string;
//   k_aoh_predict  a wavefront per block, 64 time-ordered steps per round over that string: k_predict_wave<false> (w3_predict_wave.h)
//                  with alignment 0, L_b steps instead of 8 per byte, the Counter table private to the resident wavefront;
//   k_aoh_coder    a lane per block codes from the stored probabilities and the string: no table access is left in the serial chain.
// Decode (the decoder cannot look ahead) and the sweep (configurations x blocks lanes already) stay on k_aoh.
#pragma once
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "w3_device.h"
#include "w3_generic.h"
#include "w3_sweep.h"
#include "w3_predict_wave.h"
#include "w3_aoh_plan.h"
#include "../../include/w3hip.h"

namespace w3 {

// One code table in device form.  enc: code | len << 16 per byte value.  Decode tables over the symbols sorted by (len, code): the
// codes of one length are ONE contiguous range (host validation), so at length l a prefix `code` is a symbol iff
// code - first[l] < count[l] (unsigned), and the symbol is sym[offs[l] + code - first[l]].
struct AohDev {
    uint32_t enc[256];
    uint32_t fc[17];        // first[l] | count[l] << 16   (count <= 256, first < 2^16)
    uint16_t offs[17];
    uint8_t  max_len, pad;
    uint8_t  sym[256];
};
static_assert(sizeof(AohDev) % 4 == 0, "staged to LDS a dword at a time");

struct AohCfg {
    uint8_t  ctx_bits, use_hash, code_idx, pad;
    uint32_t hash_mask, ctx_mask;
    uint64_t base, stride;      // Counter table of lane (cfg, block b): tables + base + (b - first_block) * stride
};

struct AohArgs {
    const uint8_t *in; uint64_t n;             // original bytes (stats / encode); n = original length (all modes)
    uint32_t block_size, nblocks;
    uint32_t first_block, n_lanes;             // this launch's block range
    uint32_t waves_per_cfg, first_cfg;
    const AohCfg *cfg; const AohDev *codes;
    uint8_t *tables;
    uint32_t *out_bits;                        // stats: [all configurations][nblocks]; encode: [nblocks] or null
    // encode
    uint8_t *stripes; uint32_t stripe_cap; uint32_t *out_len; uint32_t *overflow;
    // decode
    const uint8_t *cin; const uint64_t *coffs; const uint32_t *clens; uint8_t *dout;
    const DecodeJob *jobs;                     // null: lane k decodes block first_block + k whole; else job first_block + k (w3_ranges.h)
};

enum { AOH_STATS = 0, AOH_ENCODE = 1, AOH_DECODE = 2 };

__device__ __forceinline__ void aoh_stage(AohDev *s, const AohDev *g) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(g);
    uint32_t *dst = reinterpret_cast<uint32_t *>(s);
    for (uint32_t i = threadIdx.x; i < sizeof(AohDev) / 4; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// The lane's Counter table: direct (4 << ctx_bits bytes) or the exact map of leaf_slot (w3_generic.h: open addressing, key + 1 stored,
// 0 = empty, one writer), whichever the host found smaller.
struct AohTable {
    uint32_t *tbl; uint32_t use_hash, hash_mask;
    __device__ __forceinline__ uint32_t home(uint32_t ctx) const { return ((ctx * 2654435761u) ^ (ctx >> 15)) & hash_mask; }
    // continue the probe sequence behind slot h
    __device__ __forceinline__ uint32_t *walk(uint32_t h, uint32_t ctx) const {
        for (;;) {
            h = (h + 1u) & hash_mask;
            const uint32_t k = tbl[2u * h];
            if (k == ctx + 1u) return tbl + 2u * h + 1u;
            if (k == 0u) { tbl[2u * h] = ctx + 1u; return tbl + 2u * h + 1u; }
        }
    }
    // leaf_slot, with the slot's value: key and value of the first probe come in one 8-byte load
    __device__ __forceinline__ uint32_t *slot(uint32_t ctx, uint32_t &val) const {
        if (!use_hash) { val = tbl[ctx]; return tbl + ctx; }
        const uint32_t h = home(ctx);
        const uint2 kv = *reinterpret_cast<const uint2 *>(tbl + 2u * h);
        if (kv.x == ctx + 1u) { val = kv.y; return tbl + 2u * h + 1u; }
        if (kv.x == 0u) { tbl[2u * h] = ctx + 1u; val = 0u; return tbl + 2u * h + 1u; }
        uint32_t *p = walk(h, ctx);
        val = *p;
        return p;
    }
};

// The input four bytes at a time and one word ahead of its use, as BitSource reads the streams (w3_device.h): a byte read on demand
// would put a dependent global load into every few steps.  Byte k of the block is bits [8k mod 32, +8) of its word.
struct AohInput {
    const uint8_t *p; uint32_t len;
    __device__ __forceinline__ uint32_t word(uint32_t at) const {   // bytes [at, at + 4), zeros past len
        uint32_t v = 0u;
        if (at + 4u <= len) __builtin_memcpy(&v, p + at, 4);
        else for (uint32_t k = 0; k < 4u; k++) v |= (at + k < len ? (uint32_t)p[at + k] : 0u) << (8u * k);
        return v;
    }
};

template <int MODE>
__global__ void __launch_bounds__(64) k_aoh(AohArgs a) {
    __shared__ AohDev s_code;
    const uint32_t c = a.first_cfg + blockIdx.x / a.waves_per_cfg;          // one configuration per wavefront: uniform table kind and code
    const AohCfg cf = a.cfg[c];
    aoh_stage(&s_code, a.codes + cf.code_idx);
    const uint32_t lane = (blockIdx.x % a.waves_per_cfg) * 64u + threadIdx.x;
    if (lane >= a.n_lanes) return;
    const uint32_t b = a.first_block + lane;
    const uint64_t off = (uint64_t)b * a.block_size;
    const uint32_t len = (uint32_t)((a.n - off) < a.block_size ? (a.n - off) : a.block_size);
    AohTable T;
    T.tbl = reinterpret_cast<uint32_t *>(a.tables + cf.base + (uint64_t)lane * cf.stride);
    T.use_hash = cf.use_hash; T.hash_mask = cf.hash_mask;
    const uint32_t cmask = cf.ctx_mask;
    // OrderN(ctx_bits, 0) (models/ordern.rs:35-43): ctx = the last ctx_bits bits; the history starts at 0, so the first context is 0 and
    // the contexts of the first ctx_bits steps are what has been seen, zero-extended — all of it  hist & mask.
    uint32_t hist = 0u;

    if (MODE == AOH_DECODE) {
        uint32_t sb = b, dlen = len;                   // the stream, the bytes to decode and where they go: the block, or the lane's job
        uint64_t doff = off;
        if (a.jobs) { const DecodeJob jb = a.jobs[b]; sb = jb.blk; dlen = jb.len; doff = jb.dst; }
        Decoder dec;
        dec.init(a.cin + a.coffs[sb], a.clens[sb]);
        const uint32_t max_len = s_code.max_len;
        for (uint32_t i = 0; i < dlen; i++) {          // ends on the BYTE count
            uint32_t code = 0u, l = 0u, sym = 0u;
            while (l < max_len) {                      // (a stream that is not one of ours ends every symbol at max_len: the step count,
                uint32_t cv;                           //  and with it the exact map's fill, stays within what the host sized it for)
                uint32_t *sp = T.slot(hist & cmask, cv);
                const uint32_t bit = dec.decode(counter_p_packed(cv));
                *sp = counter_update_packed(cv, bit);
                hist = (hist << 1) | bit;
                code = (code << 1) | bit;
                l++;
                const uint32_t fc = s_code.fc[l];
                const uint32_t d = code - (fc & 0xFFFFu);
                if (d < (fc >> 16)) { sym = s_code.sym[s_code.offs[l] + d]; break; }
            }
            a.dout[doff + i] = (uint8_t)sym;
        }
        return;
    }

    // stats / encode: the next step's context is known from the input, so its Counter load (the exact map's first probe) is issued
    // before this step's load is waited for: two dependent-latency loads in flight instead of one.  The one hazard: the slot this step
    // writes (value, and the key when it claims an empty slot) is the one already fetched for the next step — compare the addresses
    // and forward what was written.
    typename std::conditional<MODE == AOH_ENCODE, Encoder, StatsEncoder>::type enc;
    if constexpr (MODE == AOH_ENCODE) enc.init(a.stripes + (uint64_t)b * a.stripe_cap, a.stripe_cap);
    AohInput in{a.in + off, len};
    uint32_t i = 0u, code = 0u, left = 0u;
    uint32_t w_cur = in.word(0u), w_next = in.word(4u);
    auto fetch = [&]() {                               // next byte with len != 0 (a byte with len 0 contributes no bits, as in the reference)
        while (left == 0u && i < len) {
            const uint32_t e = s_code.enc[(w_cur >> (8u * (i & 3u))) & 0xFFu];
            i++;
            if ((i & 3u) == 0u) { w_cur = w_next; w_next = in.word(i + 4u); }
            code = e & 0xFFFFu; left = e >> 16;
        }
    };
    struct Probe { uint32_t *slot; uint32_t key, val; };
    auto probe = [&](uint32_t ctx) {
        Probe p;
        if (!T.use_hash) { p.slot = T.tbl + ctx; p.key = ctx + 1u; p.val = *p.slot; }
        else { p.slot = T.tbl + 2u * T.home(ctx); const uint2 kv = *reinterpret_cast<const uint2 *>(p.slot); p.key = kv.x; p.val = kv.y; }
        return p;
    };
    fetch();
    Probe cur{nullptr, 0u, 0u};
    if (left) cur = probe(0u);
    while (left) {
        const uint32_t ctx = hist & cmask;
        const uint32_t bit = (code >> (left - 1u)) & 1u;
        left--;
        hist = (hist << 1) | bit;
        fetch();
        Probe nxt{nullptr, 0u, 0u};
        if (left) nxt = probe(hist & cmask);
        // resolve this step's probe: hit, claim an empty slot, or walk on (leaf_slot semantics)
        uint32_t *vp; uint32_t cv = cur.val;
        if (!T.use_hash) vp = cur.slot;
        else if (cur.key == ctx + 1u) vp = cur.slot + 1;
        else if (cur.key == 0u) { cur.slot[0] = ctx + 1u; vp = cur.slot + 1; cv = 0u; }
        else { vp = T.walk((uint32_t)(cur.slot - T.tbl) >> 1, ctx); cv = *vp; }
        const uint32_t upd = counter_update_packed(cv, bit);   // Model::update = adapt then advance (models/mod.rs:28-31)
        *vp = upd;
        if (nxt.slot == (T.use_hash ? vp - 1 : vp)) { nxt.key = ctx + 1u; nxt.val = upd; }
        enc.encode(bit, counter_p_packed(cv));
        cur = nxt;
    }
    if constexpr (MODE == AOH_ENCODE) {
        if (a.out_bits) a.out_bits[b] = enc.stats_bits();
        const uint32_t produced = enc.flush();
        a.out_len[b] = produced;
        if (produced > a.stripe_cap) atomicOr(a.overflow, 1u);
    } else {
        a.out_bits[(uint64_t)c * a.nblocks + b] = enc.bits;
    }
}

// Length pre-pass: L[k][b] = sum of len_k[byte] over block b for code table k, max_l[k] = the call's largest, flags[k] = 1 when some
// byte of the input has len 0 in table k (such output could not be decoded).  A wavefront per block, grid-stride; grid.y = tables.
__global__ void __launch_bounds__(64) k_aoh_lens(const uint8_t *in, uint64_t n, uint32_t block_size, uint32_t nblocks, const AohDev *codes,
                                                 uint32_t *L, uint32_t *max_l, uint32_t *flags) {
    __shared__ uint8_t s_len[256];
    const uint32_t k = blockIdx.y;
    for (uint32_t i = threadIdx.x; i < 256u; i += 64u) s_len[i] = (uint8_t)(codes[k].enc[i] >> 16);
    __syncthreads();
    uint32_t wmax = 0u, bad = 0u;
    for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const uint64_t off = (uint64_t)b * block_size;
        const uint32_t len = (uint32_t)((n - off) < block_size ? (n - off) : block_size);
        uint32_t sum = 0u;
        for (uint32_t i = threadIdx.x; i < len; i += 64u) { const uint32_t l = s_len[in[off + i]]; sum += l; bad |= l == 0u; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if (threadIdx.x == 0) L[(uint64_t)k * nblocks + b] = sum;
        wmax = max(wmax, sum);
    }
    if (threadIdx.x == 0 && wmax) atomicMax(max_l + k, wmax);
    if (bad) atomicOr(flags + k, 1u);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The two-phase form.  One batch of whole blocks [first_block, first_block + count) per launch of the three kernels (w3_aoh_plan.h).
// ---------------------------------------------------------------------------------------------------------------------------------
struct AohTwoArgs {
    const uint8_t *in; uint64_t n;
    uint32_t block_size, first_block, count;
    const AohDev *code;
    const uint32_t *L;                   // [blocks of the call] coded bits per block (k_aoh_lens)
    const uint64_t *str_off, *p_off;     // [blocks of the call] AohPlan: relative to the batch's string area / P
    uint8_t *str; uint16_t *P;
    // predict: one table per resident wavefront
    uint8_t *tables; uint64_t table_stride;
    uint32_t ctx_mask, use_hash, hash_slots;
    // coder
    uint8_t *stripes; uint32_t stripe_cap; uint32_t *out_len; uint32_t *overflow;
    uint32_t *out_bits;                  // stats: [blocks of the call]; encode: the same or null
};

// The rule of W3_PATH_AUTO, in the host's terms: the call's block count, ctx_bits and the table kind.  The two-phase form is to be taken
// for the shapes where its median beats the fused kernel's by more than the two paths' combined min - max spread in a run of
// tools/aoh_rate.py (profiles/aoh/aoh_rate_twophase.json).  UNMEASURED so far: both constants are 0, AUTO keeps the fused
// kernel for every shape, W3_PATH_TWOPHASE is the way in.
#define W3_AOH_AUTO_MAX_BLOCKS 0u         // two-phase for calls of up to this many blocks ...
#define W3_AOH_AUTO_HASH_ANY_BLOCKS 0     // ... and, when 1, at any block count where the table is the exact map
static inline bool aoh_auto_twophase(uint32_t nblocks, uint32_t ctx_bits, bool use_hash) {
    (void)ctx_bits;
    return nblocks <= W3_AOH_AUTO_MAX_BLOCKS || (W3_AOH_AUTO_HASH_ANY_BLOCKS && use_hash);
}

// 256 input bytes per round: at most 4096 bits = 128 words, the partial word carried from the round before, one more a code spills into
#define W3_AOH_TILE_WORDS 132u

__global__ void __launch_bounds__(64) k_aoh_pack(AohTwoArgs a) {
    __shared__ uint32_t s_enc[256];
    __shared__ uint32_t s_tile[W3_AOH_TILE_WORDS];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 256u; i += 64u) s_enc[i] = a.code->enc[i];
    for (uint32_t k = blockIdx.x; k < a.count; k += gridDim.x) {
        const uint32_t b = a.first_block + k;
        const uint64_t off = (uint64_t)b * a.block_size;
        const uint32_t len = (uint32_t)((a.n - off) < a.block_size ? (a.n - off) : a.block_size);
        const uint8_t *blk = a.in + off;
        uint8_t *region = a.str + a.str_off[b];
        uint32_t *out = reinterpret_cast<uint32_t *>(region + AOH_STR_PAD);
        if (lane < AOH_STR_PAD / 4u) reinterpret_cast<uint32_t *>(region)[lane] = 0u;
        for (uint32_t w = lane; w < W3_AOH_TILE_WORDS; w += 64u) s_tile[w] = 0u;
        __syncthreads();
        uint32_t q = 0u, w0 = 0u;   // bits written so far (L_b < 2^32: aoh_check); the tile's first word in the string
        for (uint32_t i0 = 0u; i0 < len; i0 += 256u) {
            const uint32_t i = i0 + 4u * lane;
            uint32_t word = 0u;
            if (i + 4u <= len) __builtin_memcpy(&word, blk + i, 4);
            else for (uint32_t j = 0; j < 4u; j++) word |= (i + j < len ? (uint32_t)blk[i + j] : 0u) << (8u * j);
            uint32_t e[4], mine = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) { e[j] = i + j < len ? s_enc[(word >> (8u * j)) & 0xFFu] : 0u; mine += e[j] >> 16; }
            uint32_t incl = mine;   // prefix sum of len[byte] over the round's bytes
#pragma unroll
            for (uint32_t d = 1u; d < 64u; d <<= 1) { const uint32_t v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
            const uint32_t total = __shfl(incl, 63, 64);
            uint64_t pos = (uint64_t)(q - 32u * w0) + (incl - mine);   // bit position inside the tile
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                // non-returning OR: the word is the same in whatever order the codes that share it arrive
                aoh_put_code(e[j] & 0xFFFFu, e[j] >> 16, pos, [&](uint64_t w, uint32_t v) { atomicOr(&s_tile[w], v); });
                pos += e[j] >> 16;
            }
            __syncthreads();
            const uint32_t qn = q + total, nfull = (qn >> 5) - w0;
            for (uint32_t w = lane; w < nfull; w += 64u) out[w0 + w] = __builtin_bswap32(s_tile[w]);   // coalesced
            const uint32_t carry = s_tile[nfull];
            __syncthreads();
            for (uint32_t w = lane; w < W3_AOH_TILE_WORDS; w += 64u) s_tile[w] = w == 0u ? carry : 0u;
            __syncthreads();
            w0 += nfull; q = qn;
        }
        // the last, partial word and the zero words behind it, to the region's end (k_aoh_coder reads one word ahead)
        const uint64_t region_words = (aoh_str_bytes(q) - AOH_STR_PAD) / 4u;
        for (uint64_t w = (uint64_t)w0 + lane; w < region_words; w += 64u) out[w] = w == w0 ? __builtin_bswap32(s_tile[0]) : 0u;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) k_aoh_predict(AohTwoArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t gt = lane_gt_mask();
    uint8_t *tbl8 = a.tables + (uint64_t)blockIdx.x * a.table_stride;
    uint32_t *tbl = reinterpret_cast<uint32_t *>(tbl8);
    uint64_t *tbl64 = reinterpret_cast<uint64_t *>(tbl8);
    const uint64_t tbl_words = a.use_hash ? 2ull * a.hash_slots + 2ull : (uint64_t)a.table_stride / 4u;
    for (uint32_t k = blockIdx.x; k < a.count; k += gridDim.x) {
        const uint32_t b = a.first_block + k;
        const uint32_t nsteps = a.L[b];
        if (nsteps == 0u) continue;   // (a block of absent symbols only: nothing to predict, and last_step would wrap)
        const uint8_t *bits = a.str + a.str_off[b] + AOH_STR_PAD;
        uint16_t *P = a.P + a.p_off[b];
        // a fresh model: every Counter (0, 0), the map empty
        for (uint64_t w = (uint64_t)lane * 4u; w < tbl_words; w += 256u) *reinterpret_cast<uint4 *>(tbl + w) = make_uint4(0u, 0u, 0u, 0u);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const uint64_t last_step = nsteps - 1u;
        uint64_t Wn = aoh_window(bits, lane < last_step ? lane : last_step);   // the string does not depend on the table: one round ahead
        for (uint64_t t0 = 0; t0 < nsteps; t0 += 64u) {
            const uint64_t t = t0 + lane;
            const bool valid = t < nsteps;
            const uint64_t W = Wn;
            Wn = aoh_window(bits, t + 64u < last_step ? t + 64u : last_step);
            const uint32_t bit = aoh_step_bit(W, t);
            const uint32_t ctx = aoh_step_ctx(W, t, a.ctx_mask);
            // the Counter's slot and its counts in ONE access: {key, n0 | n1 << 16} (exact map) or the u32 itself (direct)
            uint32_t slot, base = 0u;   // slot: index of the counts word in tbl
            if (!a.use_hash) { slot = ctx; if (valid) base = wv_load(&tbl[slot]); }
            else if (ctx == 0u) { slot = 2u * a.hash_slots + 1u; if (valid) base = wv_load(&tbl[slot]); }
            else {
                uint32_t h = (ctx * 2654435761u) ^ (ctx >> 15);
                slot = 0u;
                bool found = !valid;
                while (!found) {   // (every probe sequence ends: the map has twice as many slots as the longest block has steps)
                    h &= a.hash_slots - 1u;
                    const uint64_t kv = wv_load64(&tbl64[h]);
                    uint32_t key = (uint32_t)kv, c = (uint32_t)(kv >> 32);
                    if (key == 0u) {   // empty: claim it (a lane of this round with another context may get there first)
                        uint32_t expect = 0u;
                        __hip_atomic_compare_exchange_strong(&tbl[2u * h], &expect, ctx, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        key = expect == 0u ? ctx : expect;
                        c = 0u;   // (nobody has written counts to a slot claimed in this round: stores come at the round's end)
                    }
                    if (key == ctx) { slot = 2u * h + 1u; base = c; found = true; }
                    h++;
                }
            }
            // lanes of this round on the same Counter (they all read the same counts)
            uint64_t M = match_value<6>(slot) & __ballot(valid);
            if (__ballot(valid && (M & (M - 1ull)) != 0ull)) M = match_value<30>(slot >> (a.use_hash ? 1 : 0)) & match_value<2>(slot >> 30) & __ballot(valid);
            const uint64_t ones = __ballot(bit != 0u) & M;
            const uint32_t n1l = mbcnt64(ones), n0l = mbcnt64(M) - n1l;
            uint32_t s0 = (base & 0xFFFFu) + n0l, s1 = (base >> 16) + n1l;
            const bool last = valid && (M & gt) == 0ull;
            const uint32_t f0 = s0 + (bit ^ 1u), f1 = s1 + bit;
            uint32_t f = f0 | (f1 << 16);
            // Counter::update halves both counts when one reaches 65535 (counter.rs:22-25): replay such a context serially
            uint64_t satm = __ballot(last && (f0 >= 65535u || f1 >= 65535u));
            while (satm) {
                const int kk = __ffsll((long long)satm) - 1;
                const uint64_t Mc = readlane_u64(M, kk), Oc = readlane_u64(ones, kk);
                uint32_t st = readlane_u32(base, kk);
                uint64_t it = Mc;
                while (it) {
                    const int m = __ffsll((long long)it) - 1;
                    it &= it - 1;
                    if ((int)lane == m) { s0 = st & 0xFFFFu; s1 = st >> 16; }
                    st = counter_update_packed(st, (uint32_t)(Oc >> m) & 1u);
                }
                if ((int)lane == kk) f = st;
                satm &= satm - 1;
            }
            const uint32_t p = counter_p(s0, s1);
            if (last) wv_store(&tbl[slot], f);
            if (valid) P[t] = (uint16_t)p;   // the round's 64 probabilities: one 128-byte store (p_off is a multiple of 64 steps)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the round's stores are on their way before the next round's loads
            __builtin_amdgcn_s_waitcnt(0);
        }
    }
}

// One lane per block: the probabilities eight steps (one uint4) at a time with one load ahead, the string one word ahead.
template <bool STATS>
__global__ void __launch_bounds__(64) k_aoh_coder(AohTwoArgs a) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= a.count) return;
    const uint32_t b = a.first_block + k;
    const uint32_t L = a.L[b];
    const uint4 *P4 = reinterpret_cast<const uint4 *>(a.P + a.p_off[b]);
    const uint32_t *S = reinterpret_cast<const uint32_t *>(a.str + a.str_off[b] + AOH_STR_PAD);
    typename std::conditional<STATS, StatsEncoder, Encoder>::type enc;
    if constexpr (!STATS) enc.init(a.stripes + (uint64_t)b * a.stripe_cap, a.stripe_cap);
    uint4 pn = make_uint4(0u, 0u, 0u, 0u);
    uint32_t wn = 0u, w = 0u;
    if (L) { pn = P4[0]; wn = S[0]; }
    for (uint64_t t = 0; t < L; t += 8u) {
        const uint32_t g = (uint32_t)(t >> 3);
        const uint4 pv = pn;
        if (t + 8u < L) pn = P4[g + 1u];
        if ((g & 3u) == 0u) { w = __builtin_bswap32(wn); wn = S[(g >> 2) + 1u]; }   // (the region ends with a word past the string's last)
        const uint32_t byte = (w >> (24u - 8u * (g & 3u))) & 0xFFu;
        const uint32_t cnt = L - t < 8u ? (uint32_t)(L - t) : 8u;
        const uint32_t pp[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++)
            if (j < cnt) enc.encode((byte >> (7u - j)) & 1u, (pp[j >> 1] >> (16u * (j & 1u))) & 0xFFFFu);
    }
    if constexpr (!STATS) {
        if (a.out_bits) a.out_bits[b] = enc.stats_bits();
        const uint32_t produced = enc.flush();
        a.out_len[b] = produced;
        if (produced > a.stripe_cap) atomicOr(a.overflow, 1u);
    } else {
        a.out_bits[b] = enc.bits;
    }
}

}  // namespace w3

// ---------------------------------------------------------------------------------------------------------------------------------
// Host side: table preparation and validation (model construction, not the hot path)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace w3aoh {

// canonical (package_merge.rs:87-117): the first code of every length from the length counts (:107-109)
static inline void first_codes(const uint8_t *len, uint32_t cnt[18], uint32_t first[18]) {
    memset(cnt, 0, 18 * sizeof(uint32_t)); memset(first, 0, 18 * sizeof(uint32_t));
    for (int s = 0; s < 256; s++) if (len[s] && len[s] <= 16) cnt[len[s]]++;
    for (int l = 0; l < 16; l++) first[l + 1] = (first[l] + cnt[l]) << 1;
}

// canonical() as the driver uses it (:76): NOT bit-reversed.  Symbols of one length take consecutive codes in ascending symbol order
// (:92 sorts with sort_unstable_by: the order among equal lengths is the choice w3_huff_tables documents).
static inline void canonical(const uint8_t *lens, w3_huff_code *out) {
    uint32_t cnt[18], next[18];
    first_codes(lens, cnt, next);
    for (int s = 0; s < 256; s++) {
        out->len[s] = lens[s];
        out->code[s] = lens[s] ? (uint16_t)next[lens[s]]++ : 0;
    }
}

// w3hip.h "Validation": every len <= 16, code < 2^len, and the table is canonical(len) up to a permutation among symbols of equal length
static inline bool valid(const w3_huff_code *c) {
    if (!c) return false;
    for (int s = 0; s < 256; s++) {
        if (c->len[s] > 16) return false;
        if ((uint32_t)c->code[s] >> c->len[s]) return false;
    }
    uint32_t cnt[18], first[18];
    first_codes(c->len, cnt, first);
    uint8_t seen[16 * 256] = {0};
    for (int s = 0; s < 256; s++) {
        const uint32_t l = c->len[s];
        if (!l) continue;
        const uint32_t d = (uint32_t)c->code[s] - first[l];
        if (d >= cnt[l]) return false;                       // outside the length's contiguous range
        uint8_t &m = seen[(l - 1) * 256 + d];                // (d < 256; 16 lengths)
        if (m) return false;                                 // a code taken twice
        m = 1;
    }
    for (uint32_t l = 1; l <= 16; l++)                       // canonical codes that do not fit their length (Kraft sum above 1)
        if (cnt[l] && ((first[l] + cnt[l] - 1) >> l)) return false;
    return true;
}

static inline unsigned max_len(const w3_huff_code *c) {
    unsigned m = 0;
    for (int s = 0; s < 256; s++) m = std::max<unsigned>(m, c->len[s]);
    return m;
}

static inline void to_device_form(const w3_huff_code *c, w3::AohDev *d) {
    memset(d, 0, sizeof *d);
    uint32_t cnt[18], first[18];
    first_codes(c->len, cnt, first);
    uint32_t o = 0;
    for (uint32_t l = 1; l <= 16; l++) { d->fc[l] = first[l] | cnt[l] << 16; d->offs[l] = (uint16_t)o; o += cnt[l]; }
    for (int s = 0; s < 256; s++) {
        d->enc[s] = (uint32_t)c->code[s] | (uint32_t)c->len[s] << 16;
        if (c->len[s]) d->sym[d->offs[c->len[s]] + (c->code[s] - first[c->len[s]])] = (uint8_t)s;
    }
    d->max_len = (uint8_t)max_len(c);
}

}  // namespace w3aoh
