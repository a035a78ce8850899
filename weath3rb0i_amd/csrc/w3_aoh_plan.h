// w3_aoh_plan.h — the two-phase form of AC over Huffman (w3_aoh.h: k_aoh_pack -> k_aoh_predict -> k_aoh_coder), the part of it that is
// plain C++: the workspace layout and batch plan the host makes from the blocks' bit counts L[], and the two bit-string helpers the
// kernels share.  tests/test_aoh_plan.py compiles this file with g++ (tests/host/aoh_plan.cpp) and checks both against a literal
// restatement of the driver's loop (bin/ac-over-huffman/main.rs:79-84).  Device-annotated only under __HIPCC__.
//
// The Huffman bit string of a block: the codes of its bytes, each MSB first, one after the other; bit q of the string is bit
// 7 - (q & 7) of byte q >> 3 (so bit 31 - (q & 31) of the big-endian 32-bit word q >> 5).  In the workspace every block's string has
// AOH_STR_PAD zero bytes in front of it: the context of step t is the ctx_bits bits before t, and a fresh model's history is 0, so a
// backward window over the padding needs no first-steps special case.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define W3_AOH_HD __host__ __device__ __forceinline__
#else
#define W3_AOH_HD inline
#endif

namespace w3 {

enum : uint32_t {
    AOH_STR_PAD = 8,      // zero bytes in front of every string (the 8-byte backward window of step 0 lies inside them)
    AOH_STR_ALIGN = 16,   // every block's string region starts on such a boundary
    AOH_P_ALIGN = 64      // a block's first step in P is a multiple of this: k_aoh_predict's 128-byte stores stay aligned
};

// bytes of a block's string region: padding, ceil(L / 8) bytes of bits rounded up to whole 32-bit words (k_aoh_pack stores words),
// and one more zero word (k_aoh_coder reads one word ahead), rounded up to AOH_STR_ALIGN
W3_AOH_HD uint64_t aoh_str_bytes(uint32_t L) {
    const uint64_t words = ((uint64_t)L + 31u) / 32u + 1u;
    return (AOH_STR_PAD + 4u * words + (AOH_STR_ALIGN - 1u)) / AOH_STR_ALIGN * AOH_STR_ALIGN;
}
// steps a block takes in P
W3_AOH_HD uint64_t aoh_p_steps(uint32_t L) { return ((uint64_t)L + (AOH_P_ALIGN - 1u)) / AOH_P_ALIGN * AOH_P_ALIGN; }

// Put a code of `len` bits (0..16; code < 2^len) MSB first at bit position q of a string held as big-endian 32-bit words:
// or_word(w, v) must OR v into word w.  A code touches one word or two; OR-ing makes the result independent of the order in which
// the codes of one word arrive.
template <class OrWord>
W3_AOH_HD void aoh_put_code(uint32_t code, uint32_t len, uint64_t q, OrWord &&or_word) {
    if (len == 0u) return;
    const uint32_t sh = (uint32_t)q & 31u;
    const uint64_t v = (((uint64_t)code << (64u - len)) >> sh);   // the code's first bit at bit 63 - sh
    or_word(q >> 5, (uint32_t)(v >> 32));
    if (sh + len > 32u) or_word((q >> 5) + 1u, (uint32_t)v);
}

// The eight string bytes that end with the byte of step t, as one big-endian word.  `bits` points at the string's first byte (the
// AOH_STR_PAD zero bytes lie before it).
W3_AOH_HD uint64_t aoh_window(const uint8_t *bits, uint64_t t) {
    uint64_t raw;
    __builtin_memcpy(&raw, bits + (int64_t)(t >> 3) - 7, 8);
    return __builtin_bswap64(raw);
}
// bit t of the string, and the context of step t: the last ctx_bits bits before t (ctx_mask = 2^ctx_bits - 1, ctx_bits <= 31),
// the newest at bit 0, zeros where the block has not begun — OrderN(ctx_bits, 0)'s  hist & mask  (models/ordern.rs:35-43)
W3_AOH_HD uint32_t aoh_step_bit(uint64_t window, uint64_t t) { return (uint32_t)(window >> (7u - ((uint32_t)t & 7u))) & 1u; }
W3_AOH_HD uint32_t aoh_step_ctx(uint64_t window, uint64_t t, uint32_t ctx_mask) { return (uint32_t)(window >> (8u - ((uint32_t)t & 7u))) & ctx_mask; }

// ---------------------------------------------------------------------------------------------------------------------------------
// The plan: blocks go through the three kernels in batches of consecutive whole blocks.  A batch's workspace is its strings and
// 2 bytes per step of P (the Counter tables of the resident wavefronts do not grow with the batch: the caller takes them off the
// budget first).  Offsets are relative to the batch's own string / P area, so that every batch reuses the same memory.
// ---------------------------------------------------------------------------------------------------------------------------------
struct AohBatch { uint32_t first, count; uint64_t str_bytes, p_steps; };

struct AohPlan {
    std::vector<uint64_t> str_off;   // [nb] byte offset of block b's string REGION (padding first) in its batch's string area
    std::vector<uint64_t> p_off;     // [nb] first step of block b in its batch's P
    std::vector<AohBatch> batches;
    uint64_t max_str_bytes = 0, max_p_steps = 0;   // the largest batch's areas
    static uint64_t bytes(uint64_t str_bytes, uint64_t p_steps) { return str_bytes + 2u * p_steps; }
};

// budget: bytes one batch's strings + P may take; max_blocks: most blocks per batch (0 = no cap).  false: one block alone exceeds
// the budget (the plan is then unusable).
inline bool aoh_plan(const uint32_t *L, size_t nb, uint64_t budget, uint32_t max_blocks, AohPlan &p) {
    p.str_off.assign(nb, 0); p.p_off.assign(nb, 0); p.batches.clear();
    p.max_str_bytes = 0; p.max_p_steps = 0;
    AohBatch cur{0u, 0u, 0u, 0u};
    auto close = [&]() {
        if (cur.count == 0u) return;
        p.batches.push_back(cur);
        if (cur.str_bytes > p.max_str_bytes) p.max_str_bytes = cur.str_bytes;
        if (cur.p_steps > p.max_p_steps) p.max_p_steps = cur.p_steps;
    };
    for (size_t b = 0; b < nb; b++) {
        const uint64_t sb = aoh_str_bytes(L[b]), ps = aoh_p_steps(L[b]);
        if (AohPlan::bytes(sb, ps) > budget) return false;
        if (cur.count && (AohPlan::bytes(cur.str_bytes + sb, cur.p_steps + ps) > budget || (max_blocks && cur.count >= max_blocks))) {
            close();
            cur = AohBatch{(uint32_t)b, 0u, 0u, 0u};
        }
        if (cur.count == 0u) cur.first = (uint32_t)b;
        p.str_off[b] = cur.str_bytes; p.p_off[b] = cur.p_steps;
        cur.str_bytes += sb; cur.p_steps += ps; cur.count++;
    }
    close();
    return true;
}

}  // namespace w3
