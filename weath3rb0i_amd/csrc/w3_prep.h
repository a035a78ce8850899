// w3_prep.h — table preparation on the device: the byte histogram of a buffer (w3_histogram*, from which package_merge and the canonical
// codes of HuffHistory and AC over Huffman are built) and StationaryModel::new (w3_stationary_table_device / _staged; models/ac_hash/
// stationary.rs:14-34).  The arithmetic is plain C++, so that the host can run it too (tests/test_table_prep_cpu.py compiles this file
// with g++ and drives the 64 "lanes" of a wavefront in a loop, the input between two inaccessible pages); the kernels are below it.
//
// THE WINDOW.  Both kernels see the input [p, p + n) through a window that starts at the 16-byte boundary at or before p: window position
// w is the byte p[w - skew], skew = p & 15, valid for skew <= w < end = skew + n.  The window is cut into aligned 16-byte chunks; a chunk
// that lies inside the input is one 16-byte load, the (at most two) chunks that hold the input's first and last bytes are byte loads of
// the valid bytes only.  Nothing outside [p, p + n) is read.
//
// HISTOGRAM.  The window is dealt out in steps of 1 KiB (16 bytes per lane, one global_load_dwordx4 per wave and step reads one contiguous
// KiB, the load shape of k_partition8's histogram pass), W3_HIST_UNROLL steps per wave and turn.  Every wavefront counts into a table of
// its own in LDS with relaxed, workgroup-scope adds whose value nothing reads (ds_add_u32): only commutative adds, so the result does
// not depend on the order in which the LDS applies the adds of one instruction (DESIGN.md 3.4 is not needed).  A wave's table holds
// W3_HIST_REP copies of every counter, copy = lane % W3_HIST_REP, interleaved ([value][copy]) so that the lanes that meet the same value
// in one instruction go to W3_HIST_REP different banks instead of one address (DESIGN.md 3.9 has the measurement).  At the end the
// workgroup sums its tables into 256 uint32 partials in device memory, and k_hist256_sum adds the workgroups' partials into 256 uint64
// counts: deterministic, no device atomics.
//
// STATIONARY.  For every bit position i (0 = the MSB) there is an independent chain (c0, c1): the count of the bit's value goes up by
// one, and when it reaches 0xFFFF BOTH counts are halved, rounding up (counter.rs:20-25).  Between two halvings the chain is plain
// counting.  After a halving the count that hit is 32768 and the other at most 32767, so the next halving is at least 32767 bytes away:
// a tile of W3_STAT_TILE <= 32767 bytes holds at most one.  k_stat_count writes the number of one-bits per tile and position (8 uint16
// per tile; a streaming read).  k_stat_walk runs one wavefront per position: per batch of W3_STAT_BATCH tiles every lane takes one
// tile's count, an inclusive prefix over the lanes gives the counts behind every tile, a ballot finds the first tile in which a count
// reaches 0xFFFF; that tile's bytes are loaded (64 per lane), the position's bit plane becomes a 64-bit mask per lane, a second prefix
// and ballot find the lane and a third ballot (lane k tests byte k of that lane's 64) the byte; the halving is applied there, the rest
// of the tile is added, and the batch goes on behind that tile.  The walk is written once, over a `Wave` type that supplies the
// collectives: WaveDev (shuffles and __ballot) in the kernel, WaveHost (loops over 64 entries) on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#ifndef W3_HD
#define W3_HD __device__ __forceinline__
#endif
#ifdef __HIPCC__
#define W3_HHD __host__ __device__ __forceinline__   // what the host layer calls too: the geometry and the table
#else
#define W3_HHD W3_HD
#endif

namespace w3 {

#ifndef W3_HIST_REP               // (the three that include/w3hip.h shows too: the same values)
#define W3_HIST_REP 16u           // copies of a wave's counters (by lane % W3_HIST_REP): DESIGN.md 3.9
#define W3_STAT_TILE 4096u        // bytes per tile of the stationary walk (64 lanes x 64 bytes; <= 32767: at most one halving per tile)
#define W3_STAT_BATCH 64u         // tiles per step of the walk: one per lane
#endif
#define W3_HIST_UNROLL 4u         // KiB steps whose loads are issued together
#define W3_HIST_MAX_WG 1024u      // workgroups of k_hist256 at the most (their partials: 1 MiB)
#define W3_STAT_LIMIT 0xFFFFu     // Counter::update halves when the incremented count equals this (counter.rs:22)
static_assert(W3_STAT_TILE == 64u * 64u, "a lane takes 64 bytes of a tile: one 64-bit mask");
static_assert(W3_STAT_TILE <= 32767u, "at most one halving per tile");
static_assert(W3_STAT_BATCH == 64u, "a lane per tile of the batch");
static_assert((W3_HIST_REP & (W3_HIST_REP - 1u)) == 0 && W3_HIST_REP <= 16u, "copies: a power of two, 4 waves x 256 x copies x 4 bytes of static LDS");

W3_HD uint32_t prep_popc32(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
W3_HD uint32_t prep_popc64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
W3_HD uint32_t prep_ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }

// the window over [p, p + n)
struct PrepWindow {
    const uint8_t *p;
    uint32_t skew;   // p & 15: window position of p[0]
    uint64_t end;    // skew + n
};
W3_HHD PrepWindow prep_window(const uint8_t *p, uint64_t n) {
    PrepWindow w;
    w.p = p;
    w.skew = (uint32_t)((uintptr_t)p & 15u);
    w.end = w.skew + n;
    return w;
}

// The chunk at window position w0 (a multiple of 16).  Bytes [vlo, vhi) of it belong to the input, the others read as zero.
struct alignas(16) PrepChunk { uint32_t w[4]; };
W3_HD PrepChunk prep_load16(const PrepWindow &win, uint64_t w0, uint32_t &vlo, uint32_t &vhi) {
    PrepChunk c = {{0u, 0u, 0u, 0u}};
    vlo = w0 < win.skew ? win.skew - (uint32_t)w0 : 0u;   // (only chunk 0 starts before the input)
    vhi = w0 >= win.end ? 0u : (win.end - w0 < 16u ? (uint32_t)(win.end - w0) : 16u);
    if (vhi < vlo) vhi = vlo;
    if (vlo == 0u && vhi == 16u) {
        __builtin_memcpy(&c, __builtin_assume_aligned(win.p + (w0 - win.skew), 16), 16);
    } else {
        for (uint32_t q = 0; q < 16u; q++)   // (a fixed trip count: c stays in registers)
            if (q >= vlo && q < vhi) c.w[q >> 2] |= (uint32_t)win.p[w0 + q - win.skew] << (8u * (q & 3u));
    }
    return c;
}

// ---------------------------------------------------------------------------
// histogram
// ---------------------------------------------------------------------------
// Lane `lane` of wave gw (of nw waves): add(b) for every input byte b of its chunks.  Wave gw takes the steps [k W3_HIST_UNROLL,
// (k + 1) W3_HIST_UNROLL) for k = gw, gw + nw, ...
template <class Add>
W3_HD void hist_wave_lane(const uint8_t *p, uint64_t n, uint32_t lane, uint64_t gw, uint64_t nw, Add add) {
    const PrepWindow win = prep_window(p, n);
    const uint64_t nsteps = (win.end + 1023u) >> 10;
    for (uint64_t s = gw * W3_HIST_UNROLL; s < nsteps; s += nw * W3_HIST_UNROLL) {
        PrepChunk c[W3_HIST_UNROLL];
        uint32_t lo[W3_HIST_UNROLL], hi[W3_HIST_UNROLL];
        for (uint32_t u = 0; u < W3_HIST_UNROLL; u++) c[u] = prep_load16(win, (s + u) * 1024u + lane * 16u, lo[u], hi[u]);   // the loads first
        for (uint32_t u = 0; u < W3_HIST_UNROLL; u++) {
            if (lo[u] == 0u && hi[u] == 16u) {
                for (uint32_t q = 0; q < 16u; q++) add((c[u].w[q >> 2] >> (8u * (q & 3u))) & 0xFFu);
            } else {
                for (uint32_t q = 0; q < 16u; q++)
                    if (q >= lo[u] && q < hi[u]) add((c[u].w[q >> 2] >> (8u * (q & 3u))) & 0xFFu);
            }
        }
    }
}
// workgroups of k_hist256 for an input of n bytes (4 waves each, one turn of W3_HIST_UNROLL KiB per wave at least)
W3_HHD uint32_t hist_workgroups(uint64_t n) {
    const uint64_t turns = (n + 15u + 1024u * W3_HIST_UNROLL - 1u) / (1024u * W3_HIST_UNROLL);
    const uint64_t wg = (turns + 3u) / 4u;
    return (uint32_t)(wg < 1u ? 1u : (wg > W3_HIST_MAX_WG ? W3_HIST_MAX_WG : wg));
}

// ---------------------------------------------------------------------------
// stationary: geometry, the Counter, the table
// ---------------------------------------------------------------------------
W3_HHD uint64_t stat_tiles(const PrepWindow &win) { return (win.end + W3_STAT_TILE - 1u) / W3_STAT_TILE; }
// input bytes of tile t
W3_HD uint32_t stat_tile_len(const PrepWindow &win, uint64_t t) {
    const uint64_t a = t * W3_STAT_TILE, b = a + W3_STAT_TILE;
    const uint64_t lo = a < win.skew ? win.skew : a, hi = b < win.end ? b : win.end;
    return hi > lo ? (uint32_t)(hi - lo) : 0u;
}
// Counter::update's halving: both counts, rounding up (counter.rs:23-24)
W3_HD uint32_t stat_halve(uint32_t c) { return (c >> 1) + (c & 1u); }
// Counter::p() of (c0, c1) as StationaryModel stores it (stationary.rs:27-31; the arithmetic of w3_stationary_table)
W3_HHD uint16_t stat_table_entry(uint32_t c0, uint32_t c1) {
    const uint64_t p = (1ull << 17) * ((uint64_t)c1 + 1u) / ((uint64_t)c0 + c1 + 2u);
    return (uint16_t)((p >> 1) + (p & 1u));
}

// k_stat_count, lane `lane` of the wave that takes tile t: its 4 chunks (one contiguous KiB per wave and load).  r[j] = the one-bits
// at position 2j (low half) and 2j + 1 (high half) in its 64 bytes; bytes outside the input count as zero.
W3_HD void stat_count_lane(const PrepWindow &win, uint64_t t, uint32_t lane, uint32_t r[4]) {
    PrepChunk c[W3_STAT_TILE / 1024u];
    uint32_t lo, hi;
    for (uint32_t k = 0; k < W3_STAT_TILE / 1024u; k++) c[k] = prep_load16(win, t * W3_STAT_TILE + k * 1024u + lane * 16u, lo, hi);
    // per position four byte-wide sums side by side (SWAR: 16 words, so at most 16 each), added up at the end; position i is bit 7 - i
    uint32_t acc[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    static_assert(W3_STAT_TILE / 1024u * 4u <= 63u, "the byte-wide sums and their total stay below 256");
    for (uint32_t k = 0; k < W3_STAT_TILE / 1024u; k++)
        for (uint32_t j = 0; j < 4u; j++)
            for (uint32_t i = 0; i < 8u; i++) acc[i] += (c[k].w[j] >> (7u - i)) & 0x01010101u;
    for (uint32_t j = 0; j < 4u; j++) r[j] = ((acc[2u * j] * 0x01010101u) >> 24) | (((acc[2u * j + 1u] * 0x01010101u) >> 24) << 16);
}

// k_stat_walk, lane `lane` of the wave that reloads tile t: its 64 CONSECUTIVE bytes (window t * W3_STAT_TILE + 64 lane ...), as
// m = position pos's bit of byte k in bit k, v = byte k belongs to the input in bit k
W3_HD void stat_tile_lane_masks(const PrepWindow &win, uint64_t t, uint32_t lane, uint32_t pos, uint64_t &m, uint64_t &v) {
    PrepChunk c[4];
    uint32_t lo[4], hi[4];
    for (uint32_t k = 0; k < 4u; k++) c[k] = prep_load16(win, t * W3_STAT_TILE + lane * 64u + k * 16u, lo[k], hi[k]);
    m = 0;
    v = 0;
    for (uint32_t k = 0; k < 4u; k++) {
        for (uint32_t j = 0; j < 4u; j++) {
            // the four bytes' bits to bits 24 .. 27: bit 8b goes to 24 + b, the partial products below bit 24 do not carry
            const uint32_t four = (((c[k].w[j] >> (7u - pos)) & 0x01010101u) * 0x01020408u) >> 24;
            m |= (uint64_t)four << (16u * k + 4u * j);
        }
        v |= (uint64_t)((1u << hi[k]) - (1u << lo[k])) << (16u * k);
    }
}

// the `Wave` of the host: every per-lane value is an array of 64, every collective a loop
struct WaveHost {
    template <class T> struct Vec {
        T x[64];
        T &operator[](uint32_t l) { return x[l]; }
    };
    template <class F> void each(F f) { for (uint32_t l = 0; l < 64u; l++) f(l); }
    void incl_scan(Vec<uint32_t> &v) { for (uint32_t l = 1; l < 64u; l++) v.x[l] += v.x[l - 1]; }
    uint64_t ballot(Vec<uint32_t> &v) {
        uint64_t m = 0;
        for (uint32_t l = 0; l < 64u; l++) m |= (uint64_t)(v.x[l] != 0u) << l;
        return m;
    }
    template <class T> T get(Vec<T> &v, uint32_t l) { return v.x[l]; }
};

// The halving inside tile t: (c0, c1) is the state at the tile's first byte and a count reaches W3_STAT_LIMIT in it; on return it is the
// state behind the tile's last byte.  Returns the halvings applied (1; 0 if no count gets there, which the caller has excluded).
template <class WV>
W3_HD uint32_t stat_walk_tile(WV &wv, const PrepWindow &win, uint64_t t, uint32_t pos, uint32_t &c0, uint32_t &c1) {
    typename WV::template Vec<uint64_t> m, z;
    typename WV::template Vec<uint32_t> o1, o0, p1, p0, hit;
    wv.each([&](uint32_t l) {
        uint64_t v;
        stat_tile_lane_masks(win, t, l, pos, m[l], v);
        z[l] = v & ~m[l];
        o1[l] = p1[l] = prep_popc64(m[l]);
        o0[l] = p0[l] = prep_popc64(z[l]);
    });
    wv.incl_scan(p1);
    wv.incl_scan(p0);
    const uint32_t a0 = c0, a1 = c1;
    wv.each([&](uint32_t l) { hit[l] = (a0 + p0[l] >= W3_STAT_LIMIT || a1 + p1[l] >= W3_STAT_LIMIT) ? 1u : 0u; });
    const uint64_t lanes = wv.ballot(hit);
    const uint32_t t0 = wv.get(p0, 63u), t1 = wv.get(p1, 63u);
    if (!lanes) { c0 += t0; c1 += t1; return 0u; }
    const uint32_t g = prep_ctz64(lanes);   // the lane whose 64 bytes hold the halving
    const uint32_t g0 = wv.get(p0, g), g1 = wv.get(p1, g);
    c0 += g0 - wv.get(o0, g);
    c1 += g1 - wv.get(o1, g);
    const uint64_t mg = wv.get(m, g), zg = wv.get(z, g);
    const uint32_t b0 = c0, b1 = c1;
    wv.each([&](uint32_t l) {   // lane l: is a count there behind byte l of lane g's bytes?
        const uint64_t low = (2ull << l) - 1ull;
        hit[l] = (b0 + prep_popc64(zg & low) >= W3_STAT_LIMIT || b1 + prep_popc64(mg & low) >= W3_STAT_LIMIT) ? 1u : 0u;
    });
    const uint32_t k = prep_ctz64(wv.ballot(hit) | (1ull << 63));
    const uint64_t low = (2ull << k) - 1ull;
    c0 = stat_halve(c0 + prep_popc64(zg & low));
    c1 = stat_halve(c1 + prep_popc64(mg & low));
    c0 += prep_popc64(zg & ~low) + (t0 - g0);   // the rest of the tile: at most one halving in it
    c1 += prep_popc64(mg & ~low) + (t1 - g1);
    return 1u;
}

// The walk of position pos over [p, p + n): ones8 = k_stat_count's table of this input, (c0, c1) the entry state and on return the exit
// state (so that an input can go through in pieces), halvings += the halvings applied.
template <class WV>
W3_HD void stat_walk(WV &wv, const uint8_t *p, uint64_t n, const uint16_t *ones8, uint32_t pos, uint32_t &c0, uint32_t &c1, uint32_t &halvings) {
    const PrepWindow win = prep_window(p, n);
    const uint64_t ntiles = n ? stat_tiles(win) : 0u;
    typename WV::template Vec<uint32_t> o1, o0, p1, p0, hit;
    for (uint64_t tb = 0; tb < ntiles; tb += W3_STAT_BATCH) {
        wv.each([&](uint32_t l) {
            const uint64_t t = tb + l;
            const uint32_t ones = t < ntiles ? ones8[t * 8u + pos] : 0u;
            o1[l] = p1[l] = ones;
            o0[l] = p0[l] = t < ntiles ? stat_tile_len(win, t) - ones : 0u;
        });
        wv.incl_scan(p1);
        wv.incl_scan(p0);
        const uint32_t t0 = wv.get(p0, 63u), t1 = wv.get(p1, 63u);
        uint32_t s = 0, b0 = 0, b1 = 0;   // the batch from lane s on; (b0, b1) = the counts of the tiles before it
        for (;;) {
            const uint32_t a0 = c0, a1 = c1;
            wv.each([&](uint32_t l) { hit[l] = (l >= s && (a0 + (p0[l] - b0) >= W3_STAT_LIMIT || a1 + (p1[l] - b1) >= W3_STAT_LIMIT)) ? 1u : 0u; });
            const uint64_t tiles = wv.ballot(hit);
            if (!tiles) { c0 += t0 - b0; c1 += t1 - b1; break; }
            const uint32_t f = prep_ctz64(tiles);   // the first tile in which a count gets there
            const uint32_t f0 = wv.get(p0, f), f1 = wv.get(p1, f);
            c0 += f0 - wv.get(o0, f) - b0;
            c1 += f1 - wv.get(o1, f) - b1;
            halvings += stat_walk_tile(wv, win, tb + f, pos, c0, c1);
            b0 = f0; b1 = f1; s = f + 1u;
            if (s >= 64u) break;
        }
    }
}

}  // namespace w3

#ifdef __HIPCC__
namespace w3 {

// A wave's uint32 counters cannot overflow, and neither can a workgroup's uint32 partials: a device call is bounded by the per-call
// limit n < 2^32 - 4096 (check_args), so no count of one call exceeds 2^32 - 1.
template <uint32_t REP>
__global__ void __launch_bounds__(256) k_hist256(const uint8_t *p, uint64_t n, uint32_t *partial) {
    __shared__ uint32_t tab_[4][256u * REP];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t *tab = tab_[wv];
    for (uint32_t k = lane; k < 256u * REP; k += 64u) tab[k] = 0u;
    __syncthreads();
    uint32_t *mine = tab + (lane & (REP - 1u));
    hist_wave_lane(p, n, lane, (uint64_t)blockIdx.x * 4u + wv, (uint64_t)gridDim.x * 4u,
                   [&](uint32_t b) { (void)__hip_atomic_fetch_add(&mine[b * REP], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); });
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t w = 0; w < 4u; w++)
        for (uint32_t r = 0; r < REP; r++) sum += tab_[w][threadIdx.x * REP + r];
    partial[(size_t)blockIdx.x * 256u + threadIdx.x] = sum;
}

// counts[v] = the sum of the nwg workgroups' partials, in 64 bits: a wavefront per value v (workgroup v), lane l takes the workgroups
// l, l + 64, ... (one thread per value walking all 1,024 partials took as long as k_hist256 itself at 1e9 B)
__global__ void __launch_bounds__(64) k_hist256_sum(const uint32_t *partial, uint32_t nwg, uint64_t *counts) {
    const uint32_t v = blockIdx.x;
    uint64_t sum = 0;
    for (uint32_t g = threadIdx.x; g < nwg; g += 64u) sum += partial[(size_t)g * 256u + v];
    uint32_t lo = (uint32_t)sum, hi = (uint32_t)(sum >> 32);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = ((uint64_t)(uint32_t)__shfl_xor((int)hi, d, 64) << 32) | (uint32_t)__shfl_xor((int)lo, d, 64);
        sum += o;
        lo = (uint32_t)sum; hi = (uint32_t)(sum >> 32);
    }
    if (threadIdx.x == 0) counts[v] = sum;
}

// A wavefront per tile, grid-stride: ones8[t * 8 + i] = the one-bits at position i in tile t.
__global__ void __launch_bounds__(256) k_stat_count(const uint8_t *p, uint64_t n, uint16_t *ones8) {
    const uint32_t lane = threadIdx.x & 63u;
    const PrepWindow win = prep_window(p, n);
    const uint64_t ntiles = stat_tiles(win), stride = (uint64_t)gridDim.x * 4u;
    for (uint64_t t = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); t < ntiles; t += stride) {
        uint32_t r[4];
        stat_count_lane(win, t, lane, r);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
            for (int j = 0; j < 4; j++) r[j] += (uint32_t)__shfl_xor((int)r[j], d, 64);   // (at most 4096 per half: no carry between them)
        if (lane == 0) *(uint4 *)(ones8 + t * 8u) = make_uint4(r[0], r[1], r[2], r[3]);
    }
}

struct WaveDev {
    template <class T> struct Vec {
        T x;
        __device__ __forceinline__ T &operator[](uint32_t) { return x; }
    };
    uint32_t lane;
    template <class F> __device__ __forceinline__ void each(F f) { f(lane); }
    __device__ __forceinline__ void incl_scan(Vec<uint32_t> &v) {
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)v.x, d, 64);
            if (lane >= d) v.x += t;
        }
    }
    __device__ __forceinline__ uint64_t ballot(Vec<uint32_t> &v) { return __ballot(v.x != 0u); }
    __device__ __forceinline__ uint32_t get(Vec<uint32_t> &v, uint32_t l) { return (uint32_t)__shfl((int)v.x, (int)l, 64); }
    __device__ __forceinline__ uint64_t get(Vec<uint64_t> &v, uint32_t l) {
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v.x, (int)l, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v.x >> 32), (int)l, 64);
        return ((uint64_t)hi << 32) | lo;
    }
};

// A wavefront per bit position (workgroup i: position i).  state[2 i], state[2 i + 1] = (c0, c1) of position i, the entry state when
// the kernel starts and the exit state when it ends; state[16 + i] += the halvings.  Written by lane 0 with ordinary vector stores.
__global__ void __launch_bounds__(64) k_stat_walk(const uint8_t *p, uint64_t n, const uint16_t *ones8, uint32_t *state) {
    const uint32_t pos = blockIdx.x;
    WaveDev wv{threadIdx.x & 63u};
    uint32_t c0 = state[2u * pos], c1 = state[2u * pos + 1u], h = 0;
    stat_walk(wv, p, n, ones8, pos, c0, c1, h);
    if (wv.lane == 0) {
        state[2u * pos] = c0;
        state[2u * pos + 1u] = c1;
        state[16u + pos] += h;
    }
}

}  // namespace w3
#endif
