// w3_lmix.h — the logistic mixer stage of the two-phase encoder (gfx950): W3_NODE_MIX, definition in w3_mix_plan.h / DESIGN.md 4.
//
// The stage's inputs are known for every step before it runs: the N leaves' streams (the predict kernels wrote them), the row
// (a function of the input bits) and the coded bit.  What stays serial is the history of each weight set.
//
//   k_lmix<N>     : W3_MIX_ORDER0.  The rows of bit position j are [2^j, 2^(j+1)): the weight sets of different bit positions are
//                   disjoint, so a block is EIGHT independent chains of `len` steps each.  lane = (block in group, bit position):
//                   8 blocks per wavefront.  A block's weights live in LDS (256 rows x N x 4 B, row 0 unused: 8 KiB at N = 8,
//                   64 KiB per wavefront) beside the stretch and squash tables (8 KiB each); every weight word is read and written by
//                   exactly ONE lane, so there are no LDS atomics and no ordering between lanes to rely on (DESIGN.md 3.4's
//                   lane-order property is not used).  A chain step = one dependent LDS read of the row, N multiply-adds, one dependent
//                   table read (squash), N writes.  The leaf loads and the stretch look-ups of later steps do not depend on the chain:
//                   W3_LMIX_PF byte positions are fetched ahead of it.
//   k_lmix_one<N> : W3_MIX_ONE.  One weight set = one chain of 8 len steps per block: lane = block, weights in registers, a byte's
//                   eight probabilities of every leaf in one 16-byte load.  The slow form (a lone chain per lane).
// Both handle a ragged last block, blocks of any length >= 1 and any block count (lanes past the last block idle).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "w3_mix_plan.h"

namespace w3 {

#define W3_LMIX_BLOCKS 8   // blocks per wavefront of k_lmix
#define W3_LMIX_PF 4       // byte positions whose loads are in flight ahead of the chain

struct LmixArgs {
    const uint8_t *in;
    uint64_t n;
    uint32_t block_size, nblocks;
    const uint16_t *src[MIX_MAX_INPUTS];   // the leaves' streams, 8 x u16 per input byte, in spec leaf order
    uint16_t *P;                           // the stage's output stream (never one of src)
    const int16_t *stretch;                // [4096]
    const uint16_t *squash;                // [4095]
    uint32_t rate;
};

__device__ __forceinline__ void lmix_stage_tables(int16_t *s_str, uint16_t *s_sq, const LmixArgs &a) {
    for (uint32_t i = threadIdx.x; i < 4096u; i += 64u) s_str[i] = a.stretch[i];
    for (uint32_t i = threadIdx.x; i < 4095u; i += 64u) s_sq[i] = a.squash[i];
}

template <int N>
__global__ void __launch_bounds__(64) k_lmix(LmixArgs a) {
    __shared__ int16_t s_str[4096];
    __shared__ uint16_t s_sq[4096];
    __shared__ int32_t s_w[W3_LMIX_BLOCKS][256][N];
    lmix_stage_tables(s_str, s_sq, a);
    {
        int32_t *w = &s_w[0][0][0];
        const int32_t w0 = mix_w_init(N);
        for (uint32_t i = threadIdx.x; i < (uint32_t)(W3_LMIX_BLOCKS * 256 * N); i += 64u) w[i] = w0;
    }
    __syncthreads();
    const uint32_t bl = threadIdx.x >> 3, j = threadIdx.x & 7u;
    const uint64_t blk = (uint64_t)blockIdx.x * W3_LMIX_BLOCKS + bl;
    if (blk >= a.nblocks) return;
    const uint64_t off = blk * a.block_size;
    const uint32_t len = (uint32_t)((a.n - off) < a.block_size ? (a.n - off) : a.block_size);   // >= 1: blk < nblocks
    const uint8_t *in = a.in + off;
    uint16_t *out = a.P + off * 8u + j;

    // position base + k of the block, clamped into it (the loads of a ragged tail stay inside the block; their values are not used)
    uint32_t nx_b[W3_LMIX_PF], nx_p[W3_LMIX_PF][N];
    auto fetch = [&](uint32_t base) {
#pragma unroll
        for (int k = 0; k < W3_LMIX_PF; k++) {
            const uint32_t i = base + (uint32_t)k < len ? base + (uint32_t)k : len - 1u;
            nx_b[k] = in[i];
#pragma unroll
            for (int l = 0; l < N; l++) nx_p[k][l] = a.src[l][(off + i) * 8u + j];
        }
    };
    fetch(0u);
#pragma unroll 1
    for (uint32_t base = 0; base < len; base += W3_LMIX_PF) {
        uint32_t cb[W3_LMIX_PF];
        int32_t cs[W3_LMIX_PF][N];
#pragma unroll
        for (int k = 0; k < W3_LMIX_PF; k++) {
            cb[k] = nx_b[k];
#pragma unroll
            for (int l = 0; l < N; l++) cs[k][l] = s_str[nx_p[k][l] >> 4];
        }
        if (base + W3_LMIX_PF < len) fetch(base + W3_LMIX_PF);
#pragma unroll
        for (int k = 0; k < W3_LMIX_PF; k++) {
            if (base + (uint32_t)k >= len) break;
            const uint32_t byte = cb[k];
            const uint32_t c0 = (1u << j) | (byte >> (8u - j)), bit = (byte >> (7u - j)) & 1u;
            int32_t *wr = &s_w[bl][c0][0];
            int32_t w[N];
#pragma unroll
            for (int l = 0; l < N; l++) w[l] = wr[l];
            const int32_t p = (int32_t)s_sq[mix_predict_d(w, cs[k], N) + 2047];
            mix_train(w, cs[k], N, bit, p, a.rate);
#pragma unroll
            for (int l = 0; l < N; l++) wr[l] = w[l];
            out[(uint64_t)(base + (uint32_t)k) * 8u] = (uint16_t)p;
        }
    }
}

template <int N>
__global__ void __launch_bounds__(64) k_lmix_one(LmixArgs a) {
    __shared__ int16_t s_str[4096];
    __shared__ uint16_t s_sq[4096];
    lmix_stage_tables(s_str, s_sq, a);
    __syncthreads();
    const uint64_t blk = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (blk >= a.nblocks) return;
    const uint64_t off = blk * a.block_size;
    const uint32_t len = (uint32_t)((a.n - off) < a.block_size ? (a.n - off) : a.block_size);
    const uint8_t *in = a.in + off;
    uint4 *out = reinterpret_cast<uint4 *>(a.P) + off;
    int32_t w[N];
#pragma unroll
    for (int l = 0; l < N; l++) w[l] = mix_w_init(N);
    uint32_t nx_b = in[0];
    uint4 nx_p[N];
#pragma unroll
    for (int l = 0; l < N; l++) nx_p[l] = reinterpret_cast<const uint4 *>(a.src[l])[off];
#pragma unroll 1
    for (uint32_t i = 0; i < len; i++) {
        const uint32_t byte = nx_b;
        uint32_t q[N][4];
#pragma unroll
        for (int l = 0; l < N; l++) { q[l][0] = nx_p[l].x; q[l][1] = nx_p[l].y; q[l][2] = nx_p[l].z; q[l][3] = nx_p[l].w; }
        if (i + 1u < len) {
            nx_b = in[i + 1u];
#pragma unroll
            for (int l = 0; l < N; l++) nx_p[l] = reinterpret_cast<const uint4 *>(a.src[l])[off + i + 1u];
        }
        uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            int32_t s[N];
#pragma unroll
            for (int l = 0; l < N; l++) s[l] = s_str[((q[l][jj >> 1] >> (16 * (jj & 1))) & 0xFFFFu) >> 4];
            const int32_t p = (int32_t)s_sq[mix_predict_d(w, s, N) + 2047];
            mix_train(w, s, N, (byte >> (7 - jj)) & 1u, p, a.rate);
            o[jj >> 1] |= (uint32_t)p << (16 * (jj & 1));
        }
        out[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// W3_PATH_AUTO for a spec with a mixer node: the two-phase stage only for shapes at which its median encode time has been measured to
// beat the lane kernel's by more than the two paths' combined min - max spread (DESIGN.md 7's rule).  Measured so far
// (profiles/mixer/mixer_rate_1e8.json): 99,942,400 bytes in 64 KiB blocks — order012_mix() 34.2 ms against 2,638 ms, full_cm_mix() 87.1
// against 5,947 ms.  From that size and block size up the stage; everywhere else the lane kernel until it has been timed there
// (W3_OPT_PATH = W3_PATH_TWOPHASE asks for the stage at any size).
#define W3_LMIX_AUTO_MIN_BYTES 99942400ull
#define W3_LMIX_AUTO_MIN_BLOCK 65536ull
static inline bool lmix_auto_twophase(uint64_t nblocks, uint64_t block_size) {
    return block_size >= W3_LMIX_AUTO_MIN_BLOCK && nblocks * block_size >= W3_LMIX_AUTO_MIN_BYTES;
}

// grid: a wavefront per W3_LMIX_BLOCKS blocks (ORDER0) or per 64 blocks (ONE)
static inline void lmix_launch(const LmixArgs &a, int n_inputs, uint32_t select, hipStream_t s) {
    const dim3 blk(64);
    if (select == MIX_ORDER0) {
        const dim3 grid((a.nblocks + W3_LMIX_BLOCKS - 1) / W3_LMIX_BLOCKS);
        switch (n_inputs) {
        case 2: hipLaunchKernelGGL(k_lmix<2>, grid, blk, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_lmix<3>, grid, blk, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_lmix<4>, grid, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_lmix<5>, grid, blk, 0, s, a); break;
        case 6: hipLaunchKernelGGL(k_lmix<6>, grid, blk, 0, s, a); break;
        case 7: hipLaunchKernelGGL(k_lmix<7>, grid, blk, 0, s, a); break;
        default: hipLaunchKernelGGL(k_lmix<8>, grid, blk, 0, s, a); break;
        }
    } else {
        const dim3 grid((a.nblocks + 63u) / 64u);
        switch (n_inputs) {
        case 2: hipLaunchKernelGGL(k_lmix_one<2>, grid, blk, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_lmix_one<3>, grid, blk, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_lmix_one<4>, grid, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_lmix_one<5>, grid, blk, 0, s, a); break;
        case 6: hipLaunchKernelGGL(k_lmix_one<6>, grid, blk, 0, s, a); break;
        case 7: hipLaunchKernelGGL(k_lmix_one<7>, grid, blk, 0, s, a); break;
        default: hipLaunchKernelGGL(k_lmix_one<8>, grid, blk, 0, s, a); break;
        }
    }
}

}   // namespace w3
