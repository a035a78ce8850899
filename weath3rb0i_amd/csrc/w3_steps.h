// w3_steps.h — per-step statistics export (w3_export_steps_device / _staged) and the check of a caller's probability
// stream (w3_encode_probs_device).
//
// k_steps_rows writes, for every coded bit, one row of what the model said before that bit: every leaf's Counter::p, their
// OpinionMixer2 mix, the output of every APM stage, and optionally the bit.  Everything it reads is in HBM after the predict phase and
// the APM stages (w3_twophase.h): per input byte one 16-byte vector of 8 probabilities per leaf stream and per stage copy.  A byte's 8
// rows are 16 C contiguous output bytes (C columns of 2 bytes), a wavefront's 64 bytes 1024 C.  Index arithmetic: w3_steps_plan.h.
//   staged form (default)  the wavefront builds its tile's image of the output in LDS and writes the span with lane-contiguous 16-byte
//                          stores: every store instruction covers 1 KiB of whole lines;
//   direct form            (W3_OPT_TUNE bit 20) every lane stores its own byte's C vectors: a stride of 16 C bytes between lanes, partial
//                          lines on every store instruction.  Kept for the measurement of tools/steps_rate.py.
// Both go through the same LDS image (the 2-byte transposition), so their rows cannot differ in anything but who stores them.
#pragma once
#include <hip/hip_runtime.h>

#include "w3_predict.h"
#define W3_STEPS_HD __host__ __device__ __forceinline__
#include "w3_steps_plan.h"
#undef W3_STEPS_HD

namespace w3 {

#define W3_TUNE_STEPS_DIRECT (1u << 20)   // W3_OPT_TUNE: the row kernel's direct store form
#define W3_STEPS_GRID_CAP (256u * 8u)     // a wavefront per workgroup, 8 per CU (C = 6: 14 KiB of LDS each)

struct StepsArgs {
    const uint8_t *in; uint64_t n;
    const uint4 *leaf[W3_MAX_LEAVES];   // the leaves' streams in leaf order; null = a FrozenModel leaf (no stream: the constant 32768)
    const uint4 *apm[W3_MAX_APM];       // the stream after each APM stage
    const int16_t *stretch;             // [4096], index p >> 4 (w3_stretch_squash)
    uint4 *rows;
    uint32_t n_leaves, n_apm, n_cols, format, col_bit;
};

__device__ __forceinline__ void steps_put(uint16_t *tile, const int16_t *st, uint32_t format, uint32_t lane, uint32_t col, uint32_t C, uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) {
        const uint32_t p = (w[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
        uint32_t o = p;
        if (format != STEPS_P_U16) {
            const int32_t s = st[p >> 4];
            o = format == STEPS_STRETCH_I16 ? (uint32_t)s & 0xFFFFu : steps_f16(s);
        }
        tile[steps_tile_elem(lane, k, col, C)] = (uint16_t)o;
    }
}

// CT: the column count when it is one of the specialised ones (the loops over a byte's vectors unroll), 0 = a.n_cols at run time
template <int CT, bool STAGED>
__global__ void __launch_bounds__(64) k_steps_rows(StepsArgs a) {
    extern __shared__ uint4 steps_lds[];   // steps_lds_bytes(C): the stretch table, then the tile's image
    int16_t *st = (int16_t *)steps_lds;
    uint4 *tile4 = steps_lds + 512;
    uint16_t *tile = (uint16_t *)tile4;
    const uint32_t lane = threadIdx.x, C = CT ? (uint32_t)CT : a.n_cols;
    if (a.format != STEPS_P_U16)
        for (uint32_t i = lane; i < 1024u; i += 64u) ((uint2 *)st)[i] = ((const uint2 *)a.stretch)[i];
    __syncthreads();
    const uint64_t tiles = steps_tiles(a.n);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t cnt = steps_tile_bytes(a.n, t);
        if (lane < cnt) {
            const uint64_t g = t * W3_STEPS_TILE + lane;
            const uint4 half = make_uint4(0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u);
            uint4 acc = half;
            for (uint32_t l = 0; l < a.n_leaves; l++) {
                const uint4 v = a.leaf[l] ? a.leaf[l][g] : half;
                steps_put(tile, st, a.format, lane, l, C, v);
                acc = l ? mix_p(acc, v) : v;   // OpinionMixer2 in leaf order: a later leaf wins only on a strictly larger distance
            }
            steps_put(tile, st, a.format, lane, a.n_leaves, C, acc);
            for (uint32_t j = 0; j < a.n_apm; j++) steps_put(tile, st, a.format, lane, a.n_leaves + 1u + j, C, a.apm[j][g]);
            if (a.col_bit != W3_STEPS_NO_COL) {
                const uint32_t c = a.in[g];
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
                    const uint32_t bit = (c >> (7u - k)) & 1u;
                    tile[steps_tile_elem(lane, k, a.col_bit, C)] = (uint16_t)(a.format == STEPS_STRETCH_F16 ? steps_f16_bit(bit) : bit);
                }
            }
        }
        __syncthreads();
        uint4 *out = a.rows + steps_tile_base(t, C);
        if (STAGED) {
            const uint32_t nv = steps_tile_vecs(cnt, C);
            for (uint32_t j = 0; j < C; j++) {
                const uint32_t v = j * 64u + lane;
                if (v < nv) out[v] = tile4[v];
            }
        } else if (lane < cnt) {
            for (uint32_t j = 0; j < C; j++) {
                const uint32_t v = steps_lane_vec(lane, j, C);
                out[v] = tile4[v];
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// k_count_zero_p: how many of a caller's 8 n probabilities are 0, and the first such step.  The coders rely on p in 1 .. 65535
// (w3_coder.h): a zero makes x1 == x2, and the X-wave then spins against the O-wave.  One 16-byte vector per lane and round, counted
// with a ballot per bit position; lane 0 carries the wavefront's totals.  res[0] = count, res[1] = first step (UINT64_MAX: none).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_count_zero_p(const uint4 *p, uint64_t n, unsigned long long *res) {
    unsigned long long count = 0, first = ~0ull;
    const uint64_t rounds = (n + 255u) / 256u;
    for (uint64_t r = blockIdx.x; r < rounds; r += gridDim.x) {
        const uint64_t g = r * 256u + threadIdx.x;
        const uint4 v = g < n ? p[g] : make_uint4(~0u, ~0u, ~0u, ~0u);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t zk = 8u;   // this lane's first zero position
#pragma unroll
        for (uint32_t k = 8u; k-- > 0u;) {
            const bool z = ((w[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu) == 0u;
            count += (unsigned long long)__popcll(__ballot(z));
            if (z) zk = k;
        }
        const uint64_t any = __ballot(zk < 8u);
        if (any) {
            const int src = __ffsll((unsigned long long)any) - 1;   // lanes are in step order: the lowest one holds the round's first zero
            const uint32_t k0 = (uint32_t)__shfl((int)zk, src, 64);
            const unsigned long long step = 8ull * (r * 256u + (threadIdx.x & ~63u) + (uint32_t)src) + k0;
            if (step < first) first = step;
        }
    }
    if ((threadIdx.x & 63u) == 0u && count) { atomicAdd(&res[0], count); atomicMin(&res[1], first); }
}

}   // namespace w3
