// w3_aoh_nibble.h — the nibble logic of the sixteen-lanes-per-job decoder of AC over Huffman (w3_aoh_spec.h: k_aoh_decode_spec), the
// part of it that is plain C++: tests/test_aoh_nibble.py compiles this file with g++ (tests/host/aoh_nibble.cpp), simulates a row of
// the kernel on the CPU with it and compares with the serial decoder.  Device-annotated only under __HIPCC__.
//
// The model is OrderN(ctx_bits, 0): the context of a step is the last ctx_bits bits of the Huffman bit string (hist & ctx_mask), so the
// four steps of a NIBBLE that starts with history h can reach 1 + 2 + 4 + 8 = 15 contexts, the nodes of a binary tree:
//   node r = 1 .. 15, depth d = floor(log2 r), prefix x = r - 2^d (the d bits decoded before it): context ((h << d) | x) & ctx_mask.
// Lane r of a row loads node r's Counter when the nibble starts (a SNAPSHOT: one round trip for all 15), then the four steps run one
// after the other on the node the bits so far select.  Alignment 0 means the nibble's own updates feed its later contexts — two steps
// of one nibble may have the SAME context (ctx_bits 1: always; an all-zero string: always) — so
//   forwarding   a step takes the updated Counter of the latest earlier step of this nibble with an equal context, else the snapshot;
//   last writer  a step's update is stored only if no later step of the nibble has the same context: one store per distinct address
//                (two lanes storing to one address in one instruction have no defined order).
// With both rules the table goes through exactly the serial decoder's Counter sequence.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define W3_NIB_HD __host__ __device__ __forceinline__
#else
#define W3_NIB_HD inline
#endif

namespace w3 {

// node r (1 .. 15) of the nibble's tree
W3_NIB_HD uint32_t aoh_node_depth(uint32_t r) { return r >= 8u ? 3u : r >= 4u ? 2u : r >= 2u ? 1u : 0u; }
W3_NIB_HD uint32_t aoh_node_ctx(uint32_t hist, uint32_t r, uint32_t ctx_mask) {
    const uint32_t d = aoh_node_depth(r);
    return ((hist << d) | (r - (1u << d))) & ctx_mask;
}
// the node of step d (0 .. 3) after the nibble's first d bits `prefix`
W3_NIB_HD uint32_t aoh_path_node(uint32_t d, uint32_t prefix) { return (1u << d) + prefix; }

// the steps of the nibble taken so far: context and updated Counter of each
struct AohNibble { uint32_t ctx[4], upd[4]; };

// forwarding: the Counter step d works on — `loaded` (the snapshot) unless an earlier step of this nibble had the same context
W3_NIB_HD uint32_t aoh_forward(const AohNibble &nb, uint32_t d, uint32_t ctx, uint32_t loaded) {
    uint32_t cv = loaded;
    for (uint32_t e = 0u; e < 4u; e++)   // ascending: the latest wins  (constant trip counts: the arrays stay in registers)
        if (e < d && nb.ctx[e] == ctx) cv = nb.upd[e];
    return cv;
}

// last writer: step d of a nibble of n_steps valid steps stores its update (a job that ends inside a nibble has n_steps < 4)
W3_NIB_HD bool aoh_last_writer(const AohNibble &nb, uint32_t d, uint32_t n_steps) {
    bool last = d < n_steps;
    for (uint32_t e = 0u; e < 4u; e++)
        if (e > d && e < n_steps && nb.ctx[e] == nb.ctx[d]) last = false;
    return last;
}

// The code walk of k_aoh<AOH_DECODE> (w3_aoh.h), one decoded bit at a time: fc[l] = first[l] | count[l] << 16, offs[l], symtab as in
// AohDev.  true: a symbol ends with this bit (`sym`; 0 when the walk reached max_len without a hit: a stream that is not one of ours),
// and the walk starts over.
struct AohWalk { uint32_t code, l; };
W3_NIB_HD bool aoh_walk(AohWalk &w, uint32_t bit, const uint32_t *fc, const uint16_t *offs, const uint8_t *symtab, uint32_t max_len, uint32_t &sym) {
    w.code = (w.code << 1) | bit;
    w.l++;
    const uint32_t f = fc[w.l];
    const uint32_t d = w.code - (f & 0xFFFFu);
    const bool hit = d < (f >> 16);
    if (!hit && w.l < max_len) return false;
    sym = hit ? symtab[offs[w.l] + d] : 0u;
    w.code = 0u; w.l = 0u;
    return true;
}

// The output of a job: decoded bytes are collected in a register and leave four at a time where the address allows.  Put the byte that
// goes to an address with low bits addr_low (`last`: the job's last byte).  Returns the number n of bytes to store now — the n bytes
// that END at that address, byte k of them = bits [8k, 8k + 8) of `word` — or 0; n = 4 is one aligned word store of `word`.
struct AohOut { uint32_t buf, cnt; };
W3_NIB_HD uint32_t aoh_out_put(AohOut &o, uint32_t sym, uint32_t addr_low, bool last, uint32_t &word) {
    const uint32_t pos = addr_low & 3u;
    o.buf |= sym << (8u * pos);
    o.cnt++;
    if (pos != 3u && !last) return 0u;
    const uint32_t n = o.cnt;
    word = o.buf >> (8u * (pos + 1u - n));   // (the collected bytes are contiguous and end at pos: n <= pos + 1)
    o.buf = 0u; o.cnt = 0u;
    return n;
}

}  // namespace w3
