// w3_aoh_spec.h — the DECODER of AC over Huffman with the nibble's whole context tree loaded at once: sixteen lanes per decode job.
//
// k_aoh<AOH_DECODE> (w3_aoh.h) runs the serial loop literally, one lane per block: one dependent round trip to the Counter table per
// coded bit.  But the model is one Counter leaf over the last ctx_bits bits, so the 15 contexts the next FOUR bits can reach are known
// when the nibble starts (w3_aoh_nibble.h): lane r = 1 .. 15 of a row of sixteen loads node r's Counter — one round trip for four
// bits — and the four steps then run in registers, the Decoder state replicated in the row's lanes as in k_decode_spec
// (w3_decode_spec.h), each step taking its node's Counter by a row-local shuffle.  What k_decode_spec excludes (alignment 0: the
// nibble's own updates feed its later contexts) is handled by the two rules of w3_aoh_nibble.h: forwarding inside the nibble, and one
// store per distinct context after it.  The nibble runs across symbol boundaries, because the context does.
//
// A job is a DecodeJob {blk, len, dst}: decode stream blk for len BYTES to dout + dst (the random-access decode, w3_ranges.h); a null
// job table means job k = block k, whole.  A row takes a job, a wavefront four, a workgroup is one wavefront.  Every job has a direct
// table of 4 << ctx_bits zero-filled bytes of its own, touched by one wavefront only: plain workgroup-scope accesses through the CU's
// L1 (pl_ld32 / pl_st32), the stores of nibble k waited for before the loads of nibble k + 1.  Covered: ctx_bits <= 24 (64 MiB per
// job); above, and as the cross-check (W3_OPT_VARIANT bit 1024), the lane kernel.
#pragma once
#include "w3_aoh.h"
#include "w3_aoh_nibble.h"
#include "w3_decode_spec.h"
#include "w3_generic.h"

namespace w3 {

#define W3_AOH_SPEC_MAX_CTX_BITS 24u

struct AohSpecArgs {
    const AohDev *code;
    const DecodeJob *jobs;                     // null: job k = block k, whole
    uint64_t n; uint32_t block_size;           // original length and block size (the whole-block jobs of a null table)
    uint32_t first, count;                     // this launch's jobs [first, first + count): job first + k has table k
    uint32_t ctx_mask;
    uint8_t *tables; uint64_t stride;
    const uint8_t *cin; const uint64_t *coffs; const uint32_t *clens; uint8_t *dout;
};

static inline bool aoh_spec_covers(uint32_t ctx_bits) { return ctx_bits >= 1u && ctx_bits <= W3_AOH_SPEC_MAX_CTX_BITS; }

__global__ void __launch_bounds__(64) k_aoh_decode_spec(AohSpecArgs a) {
    __shared__ AohDev s_code;
    aoh_stage(&s_code, a.code);
    const uint32_t lane = threadIdx.x & 63u, r = lane & 15u, row0 = lane & ~15u;
    const uint32_t jl = blockIdx.x * 4u + (lane >> 4);        // this row's job inside the launch
    const bool live = jl < a.count;
    const uint32_t jc = live ? jl : a.count - 1u;
    uint32_t b = a.first + jc;
    uint64_t off = (uint64_t)b * a.block_size;
    uint32_t len = (uint32_t)((a.n - off) < a.block_size ? (a.n - off) : a.block_size);
    if (a.jobs) { const DecodeJob jb = a.jobs[b]; b = jb.blk; len = jb.len; off = jb.dst; }
    if (!live) len = 0u;
    uint32_t *tbl = reinterpret_cast<uint32_t *>(a.tables + (uint64_t)jc * a.stride);
    const uint32_t cmask = a.ctx_mask, max_len = s_code.max_len;
    const uint32_t rn = r ? r : 1u;                           // (lane 0 of a row is no node: it shadows node 1 and loads nothing)
    Decoder dec;
    dec.init(a.cin + a.coffs[b], live ? a.clens[b] : 0u);

    uint8_t *out = a.dout + off;                              // the next byte's place
    AohOut ob{0u, 0u};                                        // the bytes of the output word being filled
    uint32_t hist = 0u, left = len;
    AohWalk walk{0u, 0u};
    // wave-uniform: while any row has bytes left.  A row that is through goes on stepping on zeros; `left` guards its loads, stores
    // and output (the shuffles below must be executed by every lane).
    while (__ballot(left != 0u)) {
        uint32_t snap = 0u;
        if (left != 0u && r != 0u) snap = pl_ld32(tbl + aoh_node_ctx(hist, rn, cmask));
        AohNibble nb{};
        uint32_t node[4], prefix = 0u, n_steps = 0u;
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++) {
            node[d] = aoh_path_node(d, prefix);
            const uint32_t ctx = hist & cmask;
            const uint32_t cv = aoh_forward(nb, d, ctx, (uint32_t)__shfl((int)snap, (int)(row0 | node[d]), 64));
            const uint32_t bit = dec.decode_nz(counter_p_packed(cv));   // (Counter::p gives 1 .. 65535)
            nb.ctx[d] = ctx; nb.upd[d] = counter_update_packed(cv, bit);
            hist = (hist << 1) | bit;
            prefix = (prefix << 1) | bit;
            if (left != 0u) {                                 // (the job ends on its BYTE count: the nibble's later steps are discarded)
                n_steps = d + 1u;
                uint32_t sym;
                if (aoh_walk(walk, bit, s_code.fc, s_code.offs, s_code.sym, max_len, sym)) {
                    left--;
                    // output four bytes at a time where the address allows: a word is stored when its last byte arrives
                    uint32_t word;
                    const uint32_t nst = aoh_out_put(ob, sym, (uint32_t)(uintptr_t)out, left == 0u, word);
                    out++;
                    if (nst != 0u && r == 0u) {
                        if (nst == 4u) *reinterpret_cast<uint32_t *>(out - 4) = word;
                        else for (uint32_t k = 0; k < nst; k++) out[(int)k - (int)nst] = (uint8_t)(word >> (8u * k));
                    }
                }
            }
        }
        // one store per distinct context: the path node of the LAST step that had it
        uint32_t st_ctx = 0u, st_val = 0u;
        bool st_on = false;
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++)
            if (r == node[d] && aoh_last_writer(nb, d, n_steps)) { st_on = true; st_ctx = nb.ctx[d]; st_val = nb.upd[d]; }
        if (st_on) pl_st32(tbl + st_ctx, st_val);
        // the next nibble's loads may name what this one stored
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
    }
}

}  // namespace w3
