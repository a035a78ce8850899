// w3_export.h — the context statistics export on the device for whole inputs of any size (w3_export_counters_device / _staged and, with
// w3_export_entropy.h's key stage in front, w3_export_entropy_device / _staged): the Counter table of ONE adaptive leaf after it has seen
// the input as one stream.  In the form of w3_prep.h: the arithmetic is plain C++ over a `Wave` type (WaveDev in the kernels, WaveHost on
// the CPU: tests/test_export_cpu.py compiles this file with g++ and drives it through tests/host/export_lanes.cpp); the kernels are below
// it.  Count and replay are written ONCE, over a STEP SOURCE (below): this file has the raw source (an OrderN leaf: the contexts come
// from the input's bytes), w3_export_entropy.h the keyed one (a key per step, written by a key stage).
//
// WHY IT IS NOT SERIAL.  The context of step t (bit t of the stream, MSB first) is a pure function of the input: the bits - align stream
// bits before t and t mod 2^align (ordern.rs:35-43; zeros before bit 0).  A Counter depends on the order of its updates only where it
// halves (counter.rs:20-25): stored counts never exceed 65534, a halving leaves 32768 in the count that hit 65535, so two halvings of
// one context are at least 32767 visits apart — the argument of w3_prep.h's stationary walk, here for 2^bits contexts.
//
// THE ALGORITHM.  The input goes through in EPOCHS of E bytes, in stream order:
//   count   k_exp_count_lds<Src, REP> / k_exp_count<Src>: for every step of the epoch D[ctx] += 1 (bit 0) or 1 << 32 (bit 1): a delta
//           table of one uint64 per context, d0 in the low word and d1 in the high one.  E <= 2^28 bytes = 2^31 steps: d0 cannot carry
//           into d1.
//   apply   k_ctx_apply: for every context with D != 0 and the state S = n0 | n1 << 16: if n0 + d0 <= 65534 and n1 + d1 <= 65534 no
//           count reached 65535 inside the epoch, so no halving happened and S += D is exact; otherwise the context goes on the replay
//           list and S is left alone.  D is zeroed as it is read.
//   replay  k_exp_replay<Src>: a wavefront per listed context scans the epoch's steps in order and applies Counter::update to that
//           context's steps exactly, however many halvings the epoch holds.  A row of the source (raw: 1 KiB, 16 bytes per lane, 8,192
//           steps) holds at most one halving of the context: per-lane masks of the matching steps by bit value, a prefix over the lanes,
//           a ballot for the lane in which a count reaches 65535, Counter::update step by step over that lane's matches, adds for the
//           rest.  A block of rows (raw: eight) is only counted first (their loads in flight together, one sum over the wave); the rows
//           are walked one by one only where that sum says a count can reach 65535.
// A context is listed only if one of its counts really reaches 65535 in the epoch, every listed (context, epoch) pair holds a halving
// of its own, and a halving needs 32767 visits: at most 8 x / 32767 replays up to stream byte x (the list's size).
// (Until the two forms were merged the raw instantiations were k_ctx_count_lds<REP>, k_ctx_count and k_ctx_replay, the keyed ones
// k_expk_count_lds<REP>, k_expk_count and k_expk_replay.)
//
// THE RAW SOURCE'S LOADS.  An epoch [e0, e0 + len) of the piece [p, p + n) is seen through w3_prep.h's window (aligned 16-byte chunks,
// byte loads for the chunks that hold the epoch's first and last bytes), 1 KiB per wave and step.  A lane needs the up to 32 stream bits
// before its chunk: an unaligned 4-byte load of the bytes before it, which at an epoch's first byte are the previous epoch's last;
// within four bytes of the PIECE's start they come from `carry`, the stream bytes before the piece (zeros before byte 0 of the stream).
// Nothing outside [p, p + n) is read.  For align > 3 the context depends on the absolute bit index: abs0 is the piece's byte offset in
// the stream.
//
// WHERE IT COUNTS.  Tables of up to 2^W3_EXP_LDS_BITS contexts count in a table of the workgroup's in LDS (W3_EXP_LDS_REP copies per
// counter by lane, interleaved as k_hist256's) with relaxed adds whose value nothing reads — commutative, so the order in which the LDS
// applies the adds of one instruction does not matter (DESIGN.md 3.4 is not involved) — flushed once with one 64-bit device add per
// context the workgroup met.  Wider tables take one 64-bit device add per step.  DESIGN.md 3.10 has the measurements.
#pragma once
#include "w3_prep.h"

#ifdef __HIPCC__
#define W3_EXP_UNROLL _Pragma("unroll")   // the chunk loops: fixed trip counts, fully unrolled so that a chunk stays in registers
#else
#define W3_EXP_UNROLL
#endif

namespace w3 {

#ifndef W3_EXP_LDS_BITS
#define W3_EXP_LDS_BITS 12u            // widest table (contexts = 2^bits) that counts in LDS
#endif
#ifndef W3_EXP_LDS_REP
#define W3_EXP_LDS_REP 1u              // copies per LDS counter (by lane % copies)
#endif
#ifndef W3_EXP_EPOCH_DEFAULT
#define W3_EXP_EPOCH_DEFAULT (1u << 20)    // bytes per epoch (W3_OPT_EXPORT_EPOCH = 0): the smallest median for (19,3) at 1e9 B, DESIGN.md 3.10
#endif
#define W3_EXP_EPOCH_MAX (1u << 28)    // 2^31 steps: a delta stays below 2^31
#define W3_EXP_MAX_BITS 28u
#define W3_EXP_LDS_MAX_WG 2048u        // workgroups of the LDS form at the most (each flushes its table once)
#define W3_EXP_GLOBAL_MAX_WG 16384u
#define W3_EXP_REPLAY_ROWS 8u          // rows of a replay whose loads are issued together and whose counts are summed at once
#define W3_EXP_REPLAY_MAX_WG 8192u     // wavefronts of k_exp_replay at the most (they stride over the list)
static_assert((W3_EXP_LDS_REP & (W3_EXP_LDS_REP - 1u)) == 0 && (8u << W3_EXP_LDS_BITS) * W3_EXP_LDS_REP <= 65536u, "the workgroup's table: at most 64 KiB of LDS");
static_assert(W3_EXP_EPOCH_DEFAULT % 1024u == 0 && W3_EXP_EPOCH_DEFAULT <= W3_EXP_EPOCH_MAX, "an epoch: whole KiB, at most 2^28 bytes");

struct ExpModel { uint32_t bits, align; };   // OrderN(bits, align): bits - align history bits

// A piece of the stream on the device: [p, p + n) is stream [abs0, abs0 + n); carry = the eight stream bytes before it, big-endian (the
// last one in bits 0 .. 7; zeros where the stream has not begun); seed = HuffHistory's compressed_bits at its first byte (0 for every
// other leaf)
struct ExpPiece {
    const uint8_t *p;
    uint64_t n, abs0, carry;
    uint32_t seed;
};

// the 64 stream bits before byte i of the piece (0 <= i <= n), newest at bit 0: what the next piece's carry is for i = n
W3_HHD uint64_t exp_window(const ExpPiece &pc, uint64_t i) {
    if (i >= 8u) {
        uint64_t raw;
        __builtin_memcpy(&raw, pc.p + (i - 8u), 8);
        return __builtin_bswap64(raw);
    }
    uint64_t h = pc.carry;
    for (uint32_t k = 0; k < 7u; k++)
        if (k < i) h = (h << 8) | pc.p[k];
    return h;
}
// the 32 stream bits before byte i of the piece: the low half of exp_window, as a 4-byte load
W3_HHD uint32_t exp_hist_before(const ExpPiece &pc, uint64_t i) {
    if (i >= 4u) {
        uint32_t raw;
        __builtin_memcpy(&raw, pc.p + (i - 4u), 4);
        return __builtin_bswap32(raw);
    }
    uint32_t h = (uint32_t)pc.carry;
    for (uint32_t k = 0; k < 3u; k++)
        if (k < i) h = (h << 8) | pc.p[k];
    return h;
}

W3_HD uint32_t exp_popc(uint32_t x) { return prep_popc32(x); }
W3_HD uint32_t exp_popc(uint64_t x) { return prep_popc64(x); }
W3_HD uint32_t exp_ctz(uint32_t x) { return (uint32_t)__builtin_ctz(x); }
W3_HD uint32_t exp_ctz(uint64_t x) { return prep_ctz64(x); }

// ---------------------------------------------------------------------------
// THE STEP SOURCE.  Count and replay see "the epoch's steps" through a source `Src`, a plain struct that is a kernel argument as it
// stands.  A source cuts the epoch into ROWS of 64 lanes x a fixed number of steps (few enough that a row holds at most one halving of
// a context) and provides
//   Src::BLOCK_ROWS                                      rows of a replay whose loads are issued together and whose counts are summed at once
//   Src::Mask, Src::MASK_WORDS                           a lane's steps of one row as bits of MASK_WORDS words, in stream order from bit 0 of word 0
//   exp_rows(src)                                        its number of rows
//   exp_block_count(src, r, l, target, n0, n1)           lane l's visits of `target` by bit value in the rows r .. r + BLOCK_ROWS - 1 (rows
//                                                        behind the epoch's end are empty): the loads first, then the compares
//   exp_row_masks(src, row, l, target, z, o)             lane l's matching steps of `row` with bit 0 / bit 1
//   exp_count_wave_lane(src, lane, gw, nw, add)          add(ctx, bit) for every step of lane `lane`'s rows gw, gw + nw, ...
// The RAW source is below (an OrderN leaf: the contexts come from the input's bytes); the KEYED one is w3_export_entropy.h's.
// ---------------------------------------------------------------------------

// The chunk at position w0 of the epoch's window as a lane holds it: the bytes, which of them are input, the 32 stream bits before the
// first of those and its absolute bit index (the low bits: align <= 7).  A chunk behind the epoch's end is empty and loads nothing.
struct ExpChunk {
    PrepChunk c;
    uint32_t lo, hi, hist, bi;
};
W3_HD ExpChunk exp_chunk_load(const ExpPiece &pc, const PrepWindow &win, uint64_t e0, uint64_t w0) {
    ExpChunk x;
    x.c = prep_load16(win, w0, x.lo, x.hi);
    x.hist = x.bi = 0u;
    if (x.hi > x.lo) {
        const uint64_t i = e0 + (w0 + x.lo - win.skew);   // the piece's byte with which this lane starts
        x.hist = exp_hist_before(pc, i);
        x.bi = (uint32_t)((pc.abs0 + i) << 3);
    }
    return x;
}
// Its steps in stream order: f(ctx, bit, k) for step k = 8 q + j (byte q of the chunk, bit j from the MSB) of every input byte; jsel:
// only the bit positions j whose bit is set (0xFF: all of them).
template <class F>
W3_HD void exp_chunk_walk(const ExpChunk &x, const ExpModel &m, uint32_t jsel, F f) {
    const uint32_t hbits = m.bits - m.align;
    const uint32_t hmask = (uint32_t)((1ull << hbits) - 1ull), amask = (1u << m.align) - 1u;
    uint32_t hist = x.hist, bi = x.bi;
    W3_EXP_UNROLL
    for (uint32_t q = 0; q < 16u; q++) {
        if (q < x.lo || q >= x.hi) continue;
        const uint32_t byte = (x.c.w[q >> 2] >> (8u * (q & 3u))) & 0xFFu;
        const uint64_t word = ((uint64_t)hist << 8) | byte;
        W3_EXP_UNROLL
        for (uint32_t j = 0; j < 8u; j++) {
            if (!((jsel >> j) & 1u)) continue;
            const uint32_t h = (uint32_t)(word >> (8u - j));   // the stream bits before bit j of this byte
            f(((h & hmask) << m.align) | ((bi + j) & amask), (byte >> (7u - j)) & 1u, 8u * q + j);
        }
        hist = (uint32_t)word;
        bi += 8u;
    }
}

// The raw source: the epoch [e0, e0 + len) of the piece under OrderN m.  Rows of 1 KiB of the epoch's window, 16 bytes = 128 steps per lane.
struct ExpRawSrc {
    ExpPiece pc;
    uint64_t e0, len;
    ExpModel m;
    typedef uint64_t Mask;
    static constexpr uint32_t MASK_WORDS = 2u, BLOCK_ROWS = W3_EXP_REPLAY_ROWS;
};
W3_HD PrepWindow exp_src_window(const ExpRawSrc &s) { return prep_window(s.pc.p + s.e0, s.len); }
W3_HHD uint64_t exp_rows(const ExpRawSrc &s) { return s.len ? (prep_window(s.pc.p + s.e0, s.len).end + 1023u) >> 10 : 0u; }

template <class Add>
W3_HD void exp_count_wave_lane(const ExpRawSrc &s, uint32_t lane, uint64_t gw, uint64_t nw, Add add) {
    const PrepWindow win = exp_src_window(s);
    const uint64_t rows = exp_rows(s);
    for (uint64_t r = gw; r < rows; r += nw)
        exp_chunk_walk(exp_chunk_load(s.pc, win, s.e0, r * 1024u + lane * 16u), s.m, 0xFFu, [&](uint32_t ctx, uint32_t bit, uint32_t) { add(ctx, bit); });
}

// align >= 3: a byte starts at a multiple of 8 bits, so only bit position target & 7 of a byte can match
W3_HD uint32_t exp_replay_jsel(const ExpModel &m, uint32_t target) { return m.align >= 3u ? 1u << (target & 7u) : 0xFFu; }

W3_HD void exp_row_masks(const ExpRawSrc &s, uint64_t row, uint32_t l, uint32_t target, uint64_t (&z)[2], uint64_t (&o)[2]) {
    uint64_t z0 = 0, z1 = 0, a0 = 0, a1 = 0;   // steps 0 .. 63, 64 .. 127
    exp_chunk_walk(exp_chunk_load(s.pc, exp_src_window(s), s.e0, row * 1024u + l * 16u), s.m, exp_replay_jsel(s.m, target), [&](uint32_t ctx, uint32_t bit, uint32_t k) {
        const uint64_t hitbit = (uint64_t)(ctx == target) << (k & 63u);
        if (k < 64u) { if (bit) a0 |= hitbit; else z0 |= hitbit; }
        else { if (bit) a1 |= hitbit; else z1 |= hitbit; }
    });
    z[0] = z0; z[1] = z1; o[0] = a0; o[1] = a1;
}

// every loop has a fixed trip count and is unrolled, so that the eight named chunks stay in registers
W3_HD void exp_block_count(const ExpRawSrc &s, uint64_t r, uint32_t l, uint32_t target, uint32_t &n0, uint32_t &n1) {
    const PrepWindow win = exp_src_window(s);
    const uint32_t jsel = exp_replay_jsel(s.m, target);
    ExpChunk x0 = exp_chunk_load(s.pc, win, s.e0, (r + 0u) * 1024u + l * 16u), x1 = exp_chunk_load(s.pc, win, s.e0, (r + 1u) * 1024u + l * 16u);
    ExpChunk x2 = exp_chunk_load(s.pc, win, s.e0, (r + 2u) * 1024u + l * 16u), x3 = exp_chunk_load(s.pc, win, s.e0, (r + 3u) * 1024u + l * 16u);
    ExpChunk x4 = exp_chunk_load(s.pc, win, s.e0, (r + 4u) * 1024u + l * 16u), x5 = exp_chunk_load(s.pc, win, s.e0, (r + 5u) * 1024u + l * 16u);
    ExpChunk x6 = exp_chunk_load(s.pc, win, s.e0, (r + 6u) * 1024u + l * 16u), x7 = exp_chunk_load(s.pc, win, s.e0, (r + 7u) * 1024u + l * 16u);
    static_assert(W3_EXP_REPLAY_ROWS == 8u, "eight named chunks");
    auto count = [&](uint32_t ctx, uint32_t bit, uint32_t) {
        const uint32_t hit = ctx == target ? 1u : 0u;
        n1 += hit & bit;
        n0 += hit & (bit ^ 1u);
    };
    exp_chunk_walk(x0, s.m, jsel, count); exp_chunk_walk(x1, s.m, jsel, count); exp_chunk_walk(x2, s.m, jsel, count); exp_chunk_walk(x3, s.m, jsel, count);
    exp_chunk_walk(x4, s.m, jsel, count); exp_chunk_walk(x5, s.m, jsel, count); exp_chunk_walk(x6, s.m, jsel, count); exp_chunk_walk(x7, s.m, jsel, count);
}

// ---------------------------------------------------------------------------
// apply and replay, over any source
// ---------------------------------------------------------------------------
// apply: the delta d of one context (d != 0) onto its state s.  False: s += d was exact.  True: a count reaches 65535 inside the
// epoch — replay; s is left alone.
W3_HD bool exp_apply(uint64_t d, uint32_t &s) {
    const uint32_t n0 = (s & 0xFFFFu) + (uint32_t)d, n1 = (s >> 16) + (uint32_t)(d >> 32);   // (deltas below 2^31: no overflow)
    if (n0 >= W3_STAT_LIMIT || n1 >= W3_STAT_LIMIT) return true;
    s = n0 | (n1 << 16);
    return false;
}

// Counter::update (counter.rs:20-25); returns 1 if it halved
W3_HD uint32_t exp_counter_update(uint32_t &c0, uint32_t &c1, uint32_t bit) {
    uint32_t &c = bit ? c1 : c0;
    if (++c != W3_STAT_LIMIT) return 0u;
    c0 = stat_halve(c0);
    c1 = stat_halve(c1);
    return 1u;
}

// replay, one row: (c0, c1) is context `target`'s state at the row's first step and on return behind its last.  Returns the halvings.
template <class WV, class Src>
W3_HD uint32_t exp_replay_row(WV &wv, const Src &src, uint64_t row, uint32_t target, uint32_t &c0, uint32_t &c1) {
    typedef typename Src::Mask Mask;
    typename WV::template Vec<Mask> z[Src::MASK_WORDS], o[Src::MASK_WORDS];   // the lane's matching steps with bit 0 / bit 1
    typename WV::template Vec<uint32_t> o0, o1, p0, p1, hit;
    wv.each([&](uint32_t l) {
        Mask mz[Src::MASK_WORDS], mo[Src::MASK_WORDS];
        exp_row_masks(src, row, l, target, mz, mo);
        uint32_t n0 = 0, n1 = 0;
        W3_EXP_UNROLL
        for (uint32_t w = 0; w < Src::MASK_WORDS; w++) {
            z[w][l] = mz[w]; o[w][l] = mo[w];
            n0 += exp_popc(mz[w]); n1 += exp_popc(mo[w]);
        }
        o0[l] = p0[l] = n0;
        o1[l] = p1[l] = n1;
    });
    wv.incl_scan(p0);
    wv.incl_scan(p1);
    const uint32_t a0 = c0, a1 = c1;
    wv.each([&](uint32_t l) { hit[l] = (a0 + p0[l] >= W3_STAT_LIMIT || a1 + p1[l] >= W3_STAT_LIMIT) ? 1u : 0u; });
    const uint64_t lanes = wv.ballot(hit);
    const uint32_t t0 = wv.get(p0, 63u), t1 = wv.get(p1, 63u);
    if (!lanes) { c0 += t0; c1 += t1; return 0u; }
    const uint32_t g = prep_ctz64(lanes);   // the lane whose steps hold the halving
    const uint32_t g0 = wv.get(p0, g), g1 = wv.get(p1, g);
    c0 += g0 - wv.get(o0, g);
    c1 += g1 - wv.get(o1, g);
    uint32_t halvings = 0;
    W3_EXP_UNROLL
    for (uint32_t w = 0; w < Src::MASK_WORDS; w++) {   // that lane's matches in order (every lane walks the same values)
        const Mask zg = wv.get(z[w], g), og = wv.get(o[w], g);
        for (Mask mm = zg | og; mm; mm &= mm - 1u) halvings += exp_counter_update(c0, c1, (uint32_t)(og >> exp_ctz(mm)) & 1u);
    }
    c0 += t0 - g0;   // the rest of the row: it holds at most one halving of a context
    c1 += t1 - g1;
    return halvings;
}

// replay of context `target` over the epoch: s = its state before the epoch, on return behind it.  Returns the halvings.
template <class WV, class Src>
W3_HD uint32_t exp_replay(WV &wv, const Src &src, uint32_t target, uint32_t &s) {
    const uint64_t rows = exp_rows(src);
    uint32_t c0 = s & 0xFFFFu, c1 = s >> 16, halvings = 0;
    typename WV::template Vec<uint32_t> q0, q1;
    // BLOCK_ROWS rows at a time: their loads together, the context's visits by bit value summed over the wave; only when a count can
    // reach 65535 in them are the rows walked one by one (a halving needs 32767 visits: few blocks hold one)
    for (uint64_t r = 0; r < rows; r += Src::BLOCK_ROWS) {
        wv.each([&](uint32_t l) {
            uint32_t n0 = 0, n1 = 0;
            exp_block_count(src, r, l, target, n0, n1);
            q0[l] = n0; q1[l] = n1;
        });
        wv.incl_scan(q0);
        wv.incl_scan(q1);
        const uint32_t t0 = wv.get(q0, 63u), t1 = wv.get(q1, 63u);
        if (c0 + t0 < W3_STAT_LIMIT && c1 + t1 < W3_STAT_LIMIT) { c0 += t0; c1 += t1; continue; }
        for (uint64_t k = r; k < r + Src::BLOCK_ROWS && k < rows; k++) halvings += exp_replay_row(wv, src, k, target, c0, c1);
    }
    s = c0 | (c1 << 16);
    return halvings;
}

#ifndef __HIPCC__
// HOST BUILDS ONLY, and only until the commit before this one is no longer tested against: its host harness (tests/host/export_lanes.cpp
// as it stood there) drives this header through the two calls below.  The library never sees them.
template <class Add>
W3_HD void exp_count_wave_lane(const ExpPiece &pc, uint64_t e0, uint64_t len, const ExpModel &m, uint32_t lane, uint64_t gw, uint64_t nw, Add add) {
    exp_count_wave_lane(ExpRawSrc{pc, e0, len, m}, lane, gw, nw, add);
}
template <class WV>
W3_HD uint32_t exp_replay(WV &wv, const ExpPiece &pc, uint64_t e0, uint64_t len, const ExpModel &m, uint32_t target, uint32_t &s) {
    return exp_replay(wv, ExpRawSrc{pc, e0, len, m}, target, s);
}
#endif

// entries of the replay list that suffice up to stream byte x: a listed (context, epoch) pair holds a halving, a halving 32767 visits
W3_HHD uint64_t exp_list_cap(uint32_t bits, uint64_t x) {
    const uint64_t by_visits = x / 32767u * 8u + 8u, by_table = 1ull << bits;   // (>= 8 x / 32767, without overflow)
    return by_visits < by_table ? by_visits : by_table;
}

// stats words of the kernels
#define W3_EXP_ST_LISTED 0u     // contexts on the list of the current epoch (the count kernel zeroes it, k_ctx_apply adds)
#define W3_EXP_ST_REPLAYS 1u    // listed contexts of all epochs so far
#define W3_EXP_ST_HALVINGS 2u   // halvings the replays applied
#define W3_EXP_ST_OVERFLOW 3u   // != 0: a list longer than its bound (cannot happen; guarded, not trusted)
#define W3_EXP_ST_WORDS 4u

}  // namespace w3

#ifdef __HIPCC__
namespace w3 {

typedef unsigned long long exp_u64;

// count in the workgroup's LDS table (2 counters per context, REP copies of each), one flush
template <class Src, uint32_t REP>
__global__ void __launch_bounds__(256) k_exp_count_lds(Src src, uint32_t bits, exp_u64 *D, uint32_t *stats) {
    extern __shared__ uint32_t exp_tab[];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nctx = 1u << bits;
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[W3_EXP_ST_LISTED] = 0u;
    for (uint32_t k = threadIdx.x; k < 2u * nctx * REP; k += 256u) exp_tab[k] = 0u;
    __syncthreads();
    uint32_t *mine = exp_tab + (lane & (REP - 1u));
    exp_count_wave_lane(src, lane, (uint64_t)blockIdx.x * 4u + wv, (uint64_t)gridDim.x * 4u, [&](uint32_t ctx, uint32_t bit) {
        (void)__hip_atomic_fetch_add(&mine[(2u * ctx + bit) * REP], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    });
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < nctx; c += 256u) {
        uint32_t d0 = 0, d1 = 0;
        for (uint32_t r = 0; r < REP; r++) { d0 += exp_tab[2u * c * REP + r]; d1 += exp_tab[(2u * c + 1u) * REP + r]; }
        if (d0 | d1) (void)__hip_atomic_fetch_add(&D[c], (exp_u64)d0 | ((exp_u64)d1 << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// count with one 64-bit device add per step
template <class Src>
__global__ void __launch_bounds__(256) k_exp_count(Src src, exp_u64 *D, uint32_t *stats) {
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[W3_EXP_ST_LISTED] = 0u;
    exp_count_wave_lane(src, threadIdx.x & 63u, (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6), (uint64_t)gridDim.x * 4u,
                        [&](uint32_t ctx, uint32_t bit) {
                            (void)__hip_atomic_fetch_add(&D[ctx], bit ? 1ull << 32 : 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        });
}

// A streaming pass over D and S; the listed contexts of a wavefront are appended with one add.  The grid is whole wavefronts and the
// loop's bound a multiple of 64, so that a wavefront stays together for the ballot.
__global__ void __launch_bounds__(256) k_ctx_apply(exp_u64 *D, uint32_t *S, uint64_t nctx, uint32_t *list, uint32_t cap, uint32_t *stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u, bound = (nctx + 63u) & ~63ull;
    for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < bound; c += stride) {
        bool listed = false;
        if (c < nctx) {
            const exp_u64 d = D[c];
            if (d) {
                uint32_t s = S[c];
                listed = exp_apply(d, s);
                if (!listed) S[c] = s;
                D[c] = 0ull;
            }
        }
        const uint64_t b = __ballot(listed);
        if (b) {
            const uint32_t first = prep_ctz64(b);
            uint32_t base = 0;
            if (lane == first) base = __hip_atomic_fetch_add(&stats[W3_EXP_ST_LISTED], prep_popc64(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            base = (uint32_t)__shfl((int)base, (int)first, 64);
            if (listed) {
                const uint32_t at = base + prep_popc64(b & ((1ull << lane) - 1ull));
                if (at < cap) list[at] = (uint32_t)c;
                else stats[W3_EXP_ST_OVERFLOW] = 1u;
            }
        }
    }
}

// A wavefront per listed context (workgroup i: entries i, i + gridDim.x, ...).  Lane 0 writes with ordinary vector stores.
template <class Src>
__global__ void __launch_bounds__(64) k_exp_replay(Src src, uint32_t *S, const uint32_t *list, uint32_t cap, uint32_t *stats) {
    WaveDev wv{threadIdx.x & 63u};
    const uint32_t listed = stats[W3_EXP_ST_LISTED], count = listed < cap ? listed : cap;
    uint32_t halvings = 0;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t c = list[i];
        uint32_t s = S[c];
        halvings += exp_replay(wv, src, c, s);
        if (wv.lane == 0) S[c] = s;
    }
    if (wv.lane == 0) {
        if (halvings) (void)__hip_atomic_fetch_add(&stats[W3_EXP_ST_HALVINGS], halvings, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (blockIdx.x == 0) stats[W3_EXP_ST_REPLAYS] += count;   // (one writer per launch, launches in stream order)
    }
}

}  // namespace w3
#endif
