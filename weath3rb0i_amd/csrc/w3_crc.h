// w3_crc.h — CRC-32 per block of the container (w3_crc32_blocks*, w3_crc32_verify_device and the *_checked decodes): the arithmetic in
// plain C++, so that the host can run it too (tests/test_crc_cpu.py compiles this file with g++, drives the 64 "lanes" of a wavefront
// in a loop with the input between two inaccessible pages, and compares every value with zlib), and the two kernels.
//
// The checksum is CRC-32/ISO-HDLC, zlib.crc32: reflected polynomial 0xEDB88320, init and xor-out 0xFFFFFFFF, crc("123456789") =
// 0xCBF43926, crc("") = 0.  A remainder is kept REFLECTED (bit 31 = x^0), as every table-free CRC-32 does.
//
// A wavefront takes one SLICE (at most W3_CRC_SLICE bytes) of one segment (a block).  The slice [p, p + len) is
//   head    the bytes before the first 16-byte boundary (0 .. 15; the whole slice when it holds no aligned 16-byte chunk),
//   body    nchunks aligned chunks of 16 bytes,
//   tail    the bytes after the last chunk (0 .. 15).
// The body is dealt out 1 KiB per step, 16 bytes per lane: one global_load_dwordx4 wave-instruction reads one contiguous KiB.  The
// chunks are numbered from the END — the last chunk is lane 63's in the last step, `pad` lanes of the FIRST step have none — so every
// lane's last chunk ends (63 - lane) * 16 bytes before the body's end whatever the body's length, and the closing multipliers are six
// constants.  Lane l carries the remainder r of its own strided substream: per step r = r * x^(8 * 1008) (the other lanes' 1008 bytes
// of the KiB), then its 16 bytes go through r the usual way.  Zero chunks in front of a zero remainder change nothing, which is why the
// padding is at the front.  The lane that owns the first chunk starts from the remainder of init + head instead of 0, so init and head
// ride through the same chain and need no multiplier of their own.  At the end each lane multiplies by x^(8 * 16 * (63 - lane)), the
// wavefront xors the 64 values, and the tail bytes go through the result.  Nothing outside [p, p + len) is read: the head and the tail
// are byte loads, every chunk lies inside the body, and a lane without a chunk in the first step loads chunk 0 and discards it.
//
// Bit steps and the fixed multipliers are shift-and-xor VALU (no table, no LDS): DESIGN.md 3.8.
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#ifndef W3_HD
#define W3_HD __device__ __forceinline__
#endif

namespace w3 {

#define W3_CRC_POLY 0xEDB88320u
#define W3_CRC_SLICE 65536u       // bytes per slice (a wavefront's share of a block): DESIGN.md 3.8
#define W3_CRC_UNROLL 4u          // steps whose loads are issued together

// a segment of the explicit form: staging offset, length, and the CRC the fold compares with (ignored when nothing is compared)
struct CrcSeg { uint64_t off; uint32_t len; uint32_t want; };

// r * x (one zero bit through the remainder)
W3_HD uint32_t crc_shift1(uint32_t r) { return (r >> 1) ^ (W3_CRC_POLY & (0u - (r & 1u))); }
W3_HD uint32_t crc_byte(uint32_t r, uint8_t b) {
    r ^= b;
    for (int k = 0; k < 8; k++) r = crc_shift1(r);
    return r;
}

// The definition: bytewise, one bit at a time.
W3_HD uint32_t crc32_ref(const uint8_t *buf, size_t n) {
    uint32_t r = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) r = crc_byte(r, buf[i]);
    return r ^ 0xFFFFFFFFu;
}

// a * b in GF(2)[x] / P on reflected values (x^0 = 0x80000000).  With b a compile-time constant the b-sequence folds away.
W3_HD uint32_t gf2_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = crc_shift1(b);
    }
    return p;
}

// x^(8 n) mod P by square and multiply
W3_HD uint32_t x_pow_8n(uint64_t n) {
    uint32_t p = 0x80000000u, sq = 0x00800000u;   // x^0, x^8
    while (n) {
        if (n & 1u) p = gf2_mulmod(p, sq);
        n >>= 1;
        if (n) sq = gf2_mulmod(sq, sq);
    }
    return p;
}

// CRC of A || B from crc(A), crc(B) and |B| (init and xor-out cancel: zlib's crc32_combine)
W3_HD uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return gf2_mulmod(crc_a, x_pow_8n(len_b)) ^ crc_b; }

// the same constants at compile time
constexpr uint32_t crc_c_shift1(uint32_t r) { return (r >> 1) ^ (W3_CRC_POLY & (0u - (r & 1u))); }
constexpr uint32_t crc_c_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) { p ^= b & (0u - ((a >> i) & 1u)); b = crc_c_shift1(b); }
    return p;
}
constexpr uint32_t crc_c_pow8(uint64_t n) {
    uint32_t p = 0x80000000u, sq = 0x00800000u;
    while (n) { if (n & 1u) p = crc_c_mul(p, sq); n >>= 1; sq = crc_c_mul(sq, sq); }
    return p;
}
constexpr uint32_t kCrcX4 = crc_c_pow8(4);                  // four bytes
constexpr uint32_t kCrcX1008 = crc_c_pow8(1008);            // the other 63 lanes' bytes of a step
constexpr uint32_t kCrcXSlice = crc_c_pow8(W3_CRC_SLICE);   // a full slice (the fold's shared multiplier)

// four bytes through the remainder, the first in the low bits (little-endian load): 32 zero bits behind r ^ w, as ONE fixed multiply (three
// VALU operations per bit — extract, and, xor — against four for the shift form)
W3_HD uint32_t crc_word(uint32_t r, uint32_t w) { return gf2_mulmod(r ^ w, kCrcX4); }

// one aligned 16-byte chunk
struct alignas(16) CrcChunk { uint32_t w[4]; };
W3_HD CrcChunk crc_load16(const uint8_t *q) {
    CrcChunk c;
    __builtin_memcpy(&c, __builtin_assume_aligned(q, 16), 16);
    return c;
}
W3_HD uint32_t crc_chunk(uint32_t r, const CrcChunk &c) {
    r = crc_word(r, c.w[0]); r = crc_word(r, c.w[1]); r = crc_word(r, c.w[2]);
    return crc_word(r, c.w[3]);
}

// how a slice is dealt out (the same in every lane)
struct CrcSlicePlan {
    const uint8_t *body;   // first aligned chunk
    uint32_t head, tail;   // bytes before the body / after it
    uint32_t nchunks;      // chunks of the body
    uint32_t pad;          // lanes of the first step without a chunk
    uint32_t nsteps;       // (nchunks + pad) / 64
    uint32_t owner;        // the lane whose remainder starts from init + head: pad, or 63 for an empty body (multiplier x^0)
};
W3_HD CrcSlicePlan crc_slice_plan(const uint8_t *p, uint32_t len) {
    CrcSlicePlan pl;
    const uint32_t to_boundary = (uint32_t)((0u - (uintptr_t)p) & 15u);
    pl.head = to_boundary < len ? to_boundary : len;
    pl.nchunks = (len - pl.head) >> 4;
    if (pl.nchunks == 0) pl.head = len;   // no aligned chunk: the whole slice is head
    pl.tail = len - pl.head - 16u * pl.nchunks;
    pl.body = p + pl.head;
    pl.pad = (64u - (pl.nchunks & 63u)) & 63u;
    pl.nsteps = (pl.nchunks + pl.pad) >> 6;
    pl.owner = pl.nchunks ? pl.pad : 63u;
    return pl;
}

// Lane `lane`'s share of the slice at p: the remainder of its substream, multiplied up to the end of the body.
W3_HD uint32_t crc_slice_lane(const CrcSlicePlan &pl, const uint8_t *p, uint32_t lane) {
    uint32_t r = 0;
    if (lane == pl.owner) {
        r = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < pl.head; i++) r = crc_byte(r, p[i]);
    }
    if (pl.nsteps) {
        // step 0: lanes below pad have no chunk; they load chunk 0 (inside the body) and discard it, so that no load sits under a branch
        const bool mine = lane >= pl.pad;
        const CrcChunk c0 = crc_load16(pl.body + 16u * (size_t)(mine ? lane - pl.pad : 0u));
        if (mine) r = crc_chunk(r, c0);
        const uint8_t *q = pl.body + 16u * ((size_t)64u + lane - pl.pad);   // this lane's chunk of step 1
        uint32_t s = 1;
        for (; s + W3_CRC_UNROLL <= pl.nsteps; s += W3_CRC_UNROLL, q += 1024u * W3_CRC_UNROLL) {
            CrcChunk c[W3_CRC_UNROLL];
            for (uint32_t u = 0; u < W3_CRC_UNROLL; u++) c[u] = crc_load16(q + 1024u * u);   // the loads first: all in flight together
            for (uint32_t u = 0; u < W3_CRC_UNROLL; u++) r = crc_chunk(gf2_mulmod(r, kCrcX1008), c[u]);
        }
        for (; s < pl.nsteps; s++, q += 1024u) r = crc_chunk(gf2_mulmod(r, kCrcX1008), crc_load16(q));
    }
    // the (63 - lane) chunks of the last step behind this lane's
    const uint32_t behind = 63u - lane;
    if (behind & 1u) r = gf2_mulmod(r, crc_c_pow8(16));
    if (behind & 2u) r = gf2_mulmod(r, crc_c_pow8(32));
    if (behind & 4u) r = gf2_mulmod(r, crc_c_pow8(64));
    if (behind & 8u) r = gf2_mulmod(r, crc_c_pow8(128));
    if (behind & 16u) r = gf2_mulmod(r, crc_c_pow8(256));
    if (behind & 32u) r = gf2_mulmod(r, crc_c_pow8(512));
    return r;
}

// from the xor of the 64 lanes' shares to the slice's CRC: the tail bytes, then xor-out
W3_HD uint32_t crc_slice_finish(const CrcSlicePlan &pl, uint32_t x) {
    const uint8_t *t = pl.body + 16u * (size_t)pl.nchunks;
    for (uint32_t i = 0; i < pl.tail; i++) x = crc_byte(x, t[i]);
    return x ^ 0xFFFFFFFFu;
}

// slices a segment of seg_len bytes is cut into
constexpr uint32_t crc_slices_of(uint32_t seg_len) { return seg_len / W3_CRC_SLICE + (seg_len % W3_CRC_SLICE != 0); }

// A segment's CRC from its slices' CRCs, in order: every slice but the last is followed by whole slices and one last one, so all of
// them but the last share the multiplier x^(8 * W3_CRC_SLICE) (Horner), and the last slice's own length closes.
W3_HD uint32_t crc_fold(const uint32_t *slice_crc, uint32_t seg_len) {
    const uint32_t ns = crc_slices_of(seg_len);
    if (ns == 0) return 0;   // crc("")
    uint32_t acc = slice_crc[0];
    for (uint32_t j = 1; j + 1 < ns; j++) acc = gf2_mulmod(acc, kCrcXSlice) ^ slice_crc[j];
    if (ns > 1) acc = crc32_combine(acc, slice_crc[ns - 1], seg_len - (ns - 1) * W3_CRC_SLICE);
    return acc;
}

}  // namespace w3

#ifdef __HIPCC__
namespace w3 {

// segment k of a call: implicit (segs == nullptr: uniform blocks of block_size over n bytes, short last one) or explicit
__device__ __forceinline__ void crc_segment(const CrcSeg *segs, uint64_t n, uint32_t block_size, uint64_t k, uint64_t &off, uint32_t &len) {
    if (segs) { off = segs[k].off; len = segs[k].len; return; }
    off = k * block_size;
    len = (uint32_t)(n - off < block_size ? n - off : block_size);
}

// A wavefront per slice; slice g = segment g / spb, slice g % spb of it (spb = slices of the longest segment: a shorter one leaves its
// last entries of slice_crc unwritten, and the fold does not read them).  Grid-stride over the slices.
__global__ void __launch_bounds__(256) k_crc32_slices(const uint8_t *base, uint64_t n, uint32_t block_size, const CrcSeg *segs, uint64_t nseg,
                                                      uint32_t spb, uint32_t *slice_crc) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nsl = nseg * spb;
    const uint64_t stride = (uint64_t)gridDim.x * 4u;
    for (uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); g < nsl; g += stride) {
        const uint64_t k = spb == 1u ? g : g / spb;
        const uint32_t j = spb == 1u ? 0u : (uint32_t)(g - k * spb);
        uint64_t off;
        uint32_t len;
        crc_segment(segs, n, block_size, k, off, len);
        const uint64_t so = (uint64_t)j * W3_CRC_SLICE;
        if (so >= len) continue;   // (no such slice in this segment)
        const uint32_t sl = len - (uint32_t)so < W3_CRC_SLICE ? len - (uint32_t)so : W3_CRC_SLICE;
        const uint8_t *p = base + off + so;
        const CrcSlicePlan pl = crc_slice_plan(p, sl);
        uint32_t x = crc_slice_lane(pl, p, lane);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x ^= (uint32_t)__shfl_xor((int)x, d, 64);
        x = crc_slice_finish(pl, x);   // (every lane: the same addresses, one broadcast load each)
        if (lane == 0) slice_crc[g] = x;
    }
}

// A thread per segment: its slices' CRCs folded in order.  out != nullptr: out[k] = the CRC.  check: compared with want[k] (implicit form)
// or segs[k].want; a mismatch lowers res[0] to k (res[0] starts at ~0) and counts in res[1] — ordinary device-memory atomics.
__global__ void __launch_bounds__(256) k_crc32_fold(uint64_t n, uint32_t block_size, const CrcSeg *segs, uint64_t nseg, uint32_t spb,
                                                    const uint32_t *slice_crc, uint32_t *out, const uint32_t *want, int check,
                                                    unsigned long long *res) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nseg; k += stride) {
        uint64_t off;
        uint32_t len;
        crc_segment(segs, n, block_size, k, off, len);
        const uint32_t c = crc_fold(slice_crc + k * spb, len);
        if (out) out[k] = c;
        if (check && c != (segs ? segs[k].want : want[k])) {
            atomicMin(&res[0], (unsigned long long)k);
            atomicAdd(&res[1], 1ull);
        }
    }
}

}  // namespace w3
#endif
