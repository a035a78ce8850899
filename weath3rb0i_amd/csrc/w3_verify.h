// w3_verify.h — which blocks the sampled verification of the LDS-add rounds re-predicts (twophase_verify in w3_twophase.h,
// k_gather_blocks / k_compare_blocks in w3_predict.h), in plain C++ so that the host runs the same functions:
// tests/test_verify_schedule.py compiles this file with g++ and checks the coverage bound stated in w3hip.h (W3_OPT_VERIFY) over every
// block count up to 20,000.
//
// The nb blocks of a call (the short last one included) are cut into S contiguous ranges of floor or ceil(nb / S) blocks; sample
// slot s takes one block of range s, chosen by the call's rotation rot = call mod ceil(nb / S).  So:
//   - one call never samples a block twice (the ranges are disjoint) and never an index >= nb;
//   - any ceil(nb / S) consecutive calls of one shape take every rotation, and with it every block of every range;
//   - only the last slot can hold the short last block: the gathered sample is (S - 1) full blocks and then that one.
// The call number is counted per input SHAPE (n, block size) of a context (VerifyCalls below): calls of other shapes in between do
// not take rotations away from a shape (with one context-wide count, two shapes that alternate while ceil(nb / S) is even would each
// only ever see even or only odd rotations), and the pieces of one host call (w3_encode_blocks) all take that call's number.
// (Until round 5 slot s took block s * nb_full / S + (call mod floor(nb_full / S)), full-length blocks only: when S did not divide
// nb_full the blocks at the end of the wider gaps were never sampled — 36 of the 15,258 full blocks at 1e9 B — nor was a short last block.)
#pragma once
#include <stdint.h>
#ifndef W3_HD
#define W3_HD __device__ __forceinline__
#endif

#define W3_VERIFY_BLOCKS 16u   // sampled blocks per call, at least

// S: max(W3_VERIFY_BLOCKS, nb * v / 256) blocks, at most v x 64 MiB of input and at most nb (v = W3_OPT_VERIFY, 1 .. 256; nb >= 1)
W3_HD uint32_t verify_sample_size(uint32_t nb, uint64_t block_size, uint32_t v) {
    const uint64_t want = (uint64_t)nb * v / 256u > W3_VERIFY_BLOCKS ? (uint64_t)nb * v / 256u : W3_VERIFY_BLOCKS;
    const uint64_t cap_bytes = (uint64_t)v * (64ull << 20) / block_size;
    const uint64_t cap = cap_bytes > 1u ? cap_bytes : 1u;
    uint64_t S = want < cap ? want : cap;
    if (S > nb) S = nb;
    return (uint32_t)S;
}

// the call's rotation: call number (the context's count of encode calls) mod ceil(nb / S)
W3_HD uint32_t verify_rotation(uint64_t call, uint32_t nb, uint32_t S) {
    const uint32_t period = (uint32_t)(((uint64_t)nb + S - 1u) / S);
    return (uint32_t)(call % period);
}

// the block sample slot s (0 .. S - 1) takes under rotation rot
W3_HD uint32_t verify_block(uint32_t rot, uint32_t s, uint32_t nb, uint32_t S) {
    const uint32_t lo = (uint32_t)((uint64_t)s * nb / S), hi = (uint32_t)((uint64_t)(s + 1u) * nb / S);
    return lo + rot % (hi - lo);
}

// Call numbers for the rotation, one count per input shape (n, block size) of a context.  Host code only (plain C++: the
// harness of tests/test_verify_schedule.py runs it too).  Up to W3_VERIFY_SHAPES shapes are remembered; a shape that is new, or that
// was forgotten (the least recently used one makes room), starts at the context's count of calls.
#define W3_VERIFY_SHAPES 256u
struct VerifyCalls {
    struct Shape { uint64_t n, bs, count, used; };
    Shape sh[W3_VERIFY_SHAPES] = {};
    uint32_t n_shapes = 0;
    uint64_t clock = 0;   // calls so far, all shapes
    uint64_t next(uint64_t n, uint64_t bs) {
        clock++;
        uint32_t k = 0, lru = 0;
        for (; k < n_shapes; k++) {
            if (sh[k].n == n && sh[k].bs == bs) break;
            if (sh[k].used < sh[lru].used) lru = k;
        }
        if (k == n_shapes) {
            k = n_shapes < W3_VERIFY_SHAPES ? n_shapes++ : lru;
            sh[k].n = n; sh[k].bs = bs; sh[k].count = clock - 1u;   // (a fresh context's first call: 0)
        }
        sh[k].used = clock;
        return sh[k].count++;
    }
};
