// w3_pack.h — pack the per-block byte streams into one contiguous buffer.
// Every block stream is byte aligned (ACWriter::flush pads, io.rs:91-100), so
// packing is byte granular: wave prefix-scan of the lengths, then a
// compaction copy.  Lengths > 0 always (flush writes at least one byte).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "w3_ranges.h"

namespace w3 {

__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint64_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// Single workgroup (1024 threads = 16 waves): exclusive scan of lens[nb] into
// offs[nb]; total[0] = sum.  nb is small (N / block_size), one pass suffices.
__global__ void __launch_bounds__(1024) k_scan_lens(const uint32_t *lens, uint64_t *offs, uint64_t *total, uint32_t nb) {
    __shared__ uint64_t wave_sum[16];
    __shared__ uint64_t carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += 1024) {
        uint32_t i = base + tid;
        uint64_t v = i < nb ? lens[i] : 0;
        uint64_t inc = wave_incl_scan_u64(v);
        if (lane == 63) wave_sum[wid] = inc;
        __syncthreads();
        uint64_t wprefix = 0;
        for (int w = 0; w < wid; w++) wprefix += wave_sum[w];
        uint64_t carry = carry_s;
        if (i < nb) offs[i] = carry + wprefix + inc - v;
        __syncthreads();
        if (tid == 1023) carry_s = carry + wprefix + inc;
        __syncthreads();
    }
    if (tid == 0) total[0] = carry_s;
}

// One workgroup per block: copy stripe -> out + offs[b].  Source stripes are
// 16-byte aligned; the destination is arbitrary, so copy bytewise at the
// ragged head/tail and 16 B per lane in between when alignment allows.
__global__ void __launch_bounds__(256) k_pack(const uint8_t *stripes, uint64_t stripe_stride, const uint32_t *lens,
                                              const uint64_t *offs, uint8_t *out, uint64_t out_cap, uint32_t nb) {
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint8_t *src = stripes + (uint64_t)b * stripe_stride;
        const uint32_t len = lens[b];
        const uint64_t o = offs[b];
        if (o + len > out_cap) continue;  // host reports W3_E_NOSPACE from the total
        uint8_t *dst = out + o;
        // bytewise, coalesced: consecutive lanes -> consecutive bytes
        for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) dst[i] = src[i];
    }
}

// The random-access decode's gather (w3_decode_ranges, w3_ranges.h): piece c copies staging[src, src + len) to out[dst, dst + len).  The
// host cuts the ranges into pieces of at most 64 KiB, one workgroup each, and the grid strides over them (no launch counts more work-items
// than a few thousand workgroups).  Bytewise up to out's first dword boundary and after the last; in between, one aligned dword store per
// lane, its value funnel-shifted from the two aligned source dwords it straddles when source and destination are aligned differently.
// Those source loads reach up to 3 bytes past the piece: the staging buffer is allocated 16 bytes longer than the pieces it holds.
#define W3_GATHER_PIECE_MAX 65536u
__global__ void __launch_bounds__(256) k_gather_pieces(const uint8_t *staging, const RangePiece *pieces, uint32_t n, uint8_t *out) {
    for (uint32_t c = blockIdx.x; c < n; c += gridDim.x) {
        const RangePiece pc = pieces[c];
        const uint8_t *src = staging + pc.src;
        uint8_t *dst = out + pc.dst;
        const uint32_t len = (uint32_t)pc.len;
        const uint32_t head = min(len, (uint32_t)(-(uintptr_t)dst & 3u));
        if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
        const uint32_t nd = (len - head) >> 2;
        const uint8_t *s1 = src + head;
        uint32_t *d1 = reinterpret_cast<uint32_t *>(dst + head);
        const uint32_t sh = (uint32_t)((uintptr_t)s1 & 3u);
        const uint32_t *sa = reinterpret_cast<const uint32_t *>(s1 - sh);
        if (sh == 0u) {
            for (uint32_t k = threadIdx.x; k < nd; k += blockDim.x) d1[k] = sa[k];
        } else {
            for (uint32_t k = threadIdx.x; k < nd; k += blockDim.x) d1[k] = (uint32_t)((((uint64_t)sa[k + 1] << 32) | sa[k]) >> (8u * sh));
        }
        const uint32_t done = head + 4u * nd;
        if (threadIdx.x < len - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
    }
}

}  // namespace w3
