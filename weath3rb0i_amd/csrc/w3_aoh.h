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
#pragma once
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "w3_device.h"
#include "w3_sweep.h"
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
        Decoder dec;
        dec.init(a.cin + a.coffs[b], a.clens[b]);
        const uint32_t max_len = s_code.max_len;
        for (uint32_t i = 0; i < len; i++) {           // ends on the block's BYTE count
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
            a.dout[off + i] = (uint8_t)sym;
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
