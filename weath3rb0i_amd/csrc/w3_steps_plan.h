// w3_steps_plan.h — the arithmetic of the per-step statistics export (w3_steps.h, w3_export_steps_device / _staged) in plain C++ (no HIP;
// tests/test_steps_cpu.py compiles it with g++): the columns of a row, where a step's element lies, how a wavefront's tile of 64 input
// bytes maps to its span of the output, the F16 form of a stretch value, and the pieces of the staged call.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

#ifndef W3_STEPS_HD
#define W3_STEPS_HD inline
#define W3_STEPS_HD_OWN
#endif

namespace w3 {

enum { STEPS_P_U16 = 0, STEPS_STRETCH_I16 = 1, STEPS_STRETCH_F16 = 2, STEPS_N_FORMATS = 3 };   // (= W3_STEPS_* of include/w3hip.h)
enum { STEPS_COL_BIT = 1u };
#define W3_STEPS_TILE 64u          // input bytes per tile: one per lane of a wavefront
#define W3_STEPS_NO_COL 0xFFFFFFFFu

// Columns of a row, in order: one per leaf (the spec's postfix leaf order, frozen leaves included), the mix of the leaves (the root
// before any APM stage), one per APM stage in chain order — the last of these model columns is what the coder is given — and, with
// STEPS_COL_BIT, the coded bit.  (The fields of w3_steps_layout, include/w3hip.h.)
struct StepsLayout { uint32_t n_cols, n_leaves, col_mix, col_apm0, n_apm, col_final, col_bit, elem_bytes; };
inline bool steps_layout(uint32_t n_leaves, uint32_t n_apm, uint32_t format, uint32_t flags, StepsLayout &o) {
    if (format >= STEPS_N_FORMATS || (flags & ~(uint32_t)STEPS_COL_BIT) || n_leaves == 0) return false;
    o.n_leaves = n_leaves; o.n_apm = n_apm;
    o.col_mix = n_leaves;
    o.col_apm0 = n_apm ? n_leaves + 1 : W3_STEPS_NO_COL;
    o.col_final = n_leaves + n_apm;
    o.col_bit = (flags & STEPS_COL_BIT) ? n_leaves + 1 + n_apm : W3_STEPS_NO_COL;
    o.n_cols = n_leaves + 1 + n_apm + ((flags & STEPS_COL_BIT) ? 1u : 0u);
    o.elem_bytes = 2;
    return true;
}

// Row t = 8 i + k: input byte i, bit k (0 = the MSB).  Elements are 2 bytes; rows are C of them, one after the other.
W3_STEPS_HD uint64_t steps_row(uint64_t i, uint32_t k) { return 8u * i + k; }
W3_STEPS_HD uint64_t steps_elem(uint64_t row, uint32_t col, uint32_t C) { return row * C + col; }
W3_STEPS_HD uint64_t steps_rows_bytes(uint64_t n, uint32_t C) { return 8u * n * C * 2u; }

// A tile is 64 consecutive input bytes, lane l taking byte 64 tile + l: 512 rows = 1024 C contiguous output bytes = 64 C vectors of 16.
// In the tile's LDS image (2-byte elements, the layout of the output itself) lane l, bit k, column c lies at steps_tile_elem; the image
// leaves as vectors v = 0 .. steps_tile_vecs(cnt, C), vector v going to output vector steps_tile_base(tile, C) + v (cnt: the bytes of the
// tile, 64 but for a ragged last one).  The direct form stores lane l's own C vectors, steps_lane_vec(l, j, C) for j < C, instead.
W3_STEPS_HD uint64_t steps_tiles(uint64_t n) { return (n + W3_STEPS_TILE - 1u) / W3_STEPS_TILE; }
W3_STEPS_HD uint32_t steps_tile_bytes(uint64_t n, uint64_t tile) { const uint64_t left = n - tile * W3_STEPS_TILE; return left < W3_STEPS_TILE ? (uint32_t)left : W3_STEPS_TILE; }
W3_STEPS_HD uint32_t steps_tile_elem(uint32_t lane, uint32_t k, uint32_t col, uint32_t C) { return (lane * 8u + k) * C + col; }
W3_STEPS_HD uint32_t steps_tile_vecs(uint32_t cnt, uint32_t C) { return cnt * C; }
W3_STEPS_HD uint64_t steps_tile_base(uint64_t tile, uint32_t C) { return tile * W3_STEPS_TILE * C; }
W3_STEPS_HD uint32_t steps_lane_vec(uint32_t lane, uint32_t j, uint32_t C) { return lane * C + j; }
W3_STEPS_HD uint32_t steps_lds_bytes(uint32_t C) { return 8192u + W3_STEPS_TILE * 16u * C; }   // the stretch table, then the tile's image

// stretch value v (-2047 .. 2047) / 256 as IEEE binary16, exact: |v| < 2^11 fits the significand, and the division is an exponent shift
// that stays in the normal range (2^-8 .. 2^3).
W3_STEPS_HD uint16_t steps_f16(int32_t v) {
    if (v == 0) return 0;
    const uint32_t sign = v < 0 ? 0x8000u : 0u, m = (uint32_t)(v < 0 ? -v : v);
    const uint32_t e = 31u - (uint32_t)__builtin_clz(m);   // floor(log2 m), 0 .. 10
    return (uint16_t)(sign | ((e + 7u) << 10) | ((m << (10u - e)) & 0x3FFu));   // m 2^-8 = 1.f x 2^(e - 8); bias 15
}
W3_STEPS_HD uint16_t steps_f16_bit(uint32_t bit) { return bit ? 0x3C00u : 0u; }   // 1.0 / 0.0

// Workgroups (a wavefront each) of the row kernel: a persistent grid that strides over the tiles.
inline uint32_t steps_grid(uint64_t tiles, uint32_t cap) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), cap); }

// The staged call's pieces: whole blocks, `run_blocks` of them per piece (the last piece takes what is left, a short last block included).
inline uint64_t steps_piece_len(uint64_t n, uint64_t block_size, uint64_t run_blocks, uint64_t o0) { return std::min<uint64_t>(run_blocks * block_size, n - o0); }

}   // namespace w3

#ifdef W3_STEPS_HD_OWN
#undef W3_STEPS_HD
#undef W3_STEPS_HD_OWN
#endif
