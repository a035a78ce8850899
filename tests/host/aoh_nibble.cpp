// A row of k_aoh_decode_spec (weath3rb0i_amd/csrc/w3_aoh_spec.h) simulated on the CPU with the kernel's own nibble logic
// (csrc/w3_aoh_nibble.h: node -> context, forwarding, the last-writer rule, the code walk) and the oracle's Counter and arithmetic
// decoder: per nibble 15 SNAPSHOT loads from a table array, four steps with forwarding, the stores after the nibble.
// Built on demand by tests/test_aoh_nibble.py:  gcc -c oracle/w3_oracle.c;  g++ -shared -I oracle tests/host/aoh_nibble.cpp w3_oracle.o
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../weath3rb0i_amd/csrc/w3_aoh_nibble.h"
#include "w3_oracle.h"

namespace {

// the decode tables of AohDev (csrc/w3_aoh.h) from a canonical (code, len) table: the codes of one length are one contiguous range
struct Tables { uint32_t fc[17]; uint16_t offs[17]; uint8_t sym[256]; uint32_t max_len; };

Tables make_tables(const uint16_t *code, const uint8_t *len) {
    Tables t;
    memset(&t, 0, sizeof t);
    uint32_t first[17], cnt[17] = {0};
    for (int l = 0; l < 17; l++) first[l] = 0xFFFFFFFFu;
    for (int s = 0; s < 256; s++) {
        const uint32_t l = len[s];
        if (!l) continue;
        cnt[l]++;
        if (code[s] < first[l]) first[l] = code[s];
        if (l > t.max_len) t.max_len = l;
    }
    uint32_t o = 0;
    for (uint32_t l = 1; l <= 16; l++) {
        if (!cnt[l]) first[l] = 0;
        t.fc[l] = first[l] | cnt[l] << 16; t.offs[l] = (uint16_t)o; o += cnt[l];
    }
    for (int s = 0; s < 256; s++)
        if (len[s]) t.sym[t.offs[len[s]] + (code[s] - first[len[s]])] = (uint8_t)s;
    return t;
}

uint32_t counter_p(uint32_t c) { w3o_counter k; k.data[0] = (uint16_t)c; k.data[1] = (uint16_t)(c >> 16); return w3o_counter_p(&k); }
uint32_t counter_update(uint32_t c, uint32_t bit) {
    w3o_counter k; k.data[0] = (uint16_t)c; k.data[1] = (uint16_t)(c >> 16);
    w3o_counter_update(&k, (uint8_t)bit);
    return (uint32_t)k.data[0] | (uint32_t)k.data[1] << 16;
}

}  // namespace

// Decode `stream` for job_len bytes into out (through the kernel's output buffering, aoh_out_put: the low bits of `out` decide which
// bytes leave as aligned words; *word_stores counts those).  variant: 0 = the kernel's rules; 1 = every path node stores (no last-writer rule; the
// stores of one nibble land in descending step order, one of the orders the hardware may take); 2 = no forwarding.
// counts: [0] nibbles, [1] full nibbles (four valid steps), [2] full nibbles in which two steps had the same context.
// Returns 0, -1 when a path node's snapshot context (aoh_node_ctx) is not the step's context, -2 for a misaligned word store.
extern "C" int aoh_nibble_decode(const uint16_t *code, const uint8_t *len, uint8_t ctx_bits, const uint8_t *stream, size_t stream_len,
                                 size_t job_len, uint8_t *out, int variant, uint64_t counts[3], uint64_t *word_stores) {
    using namespace w3;
    const Tables t = make_tables(code, len);
    const uint32_t mask = (uint32_t)((1ull << ctx_bits) - 1ull);
    uint32_t *table = (uint32_t *)calloc((size_t)1 << ctx_bits, 4);   // zero-filled, direct
    w3o_reader rd; w3o_ac ac;
    w3o_reader_init(&rd, stream, stream_len);
    w3o_ac_new_decoder(&ac, &rd);
    counts[0] = counts[1] = counts[2] = 0;
    uint32_t hist = 0;
    size_t left = job_len, i = 0;
    AohWalk walk{0u, 0u};
    AohOut ob{0u, 0u};
    *word_stores = 0;
    int rc = 0;
    while (left) {
        uint32_t snap[16] = {0}, snap_ctx[16] = {0};
        for (uint32_t r = 1; r < 16; r++) { snap_ctx[r] = aoh_node_ctx(hist, r, mask); snap[r] = table[snap_ctx[r]]; }
        AohNibble nb{};
        uint32_t prefix = 0, n_steps = 0;
        for (uint32_t d = 0; d < 4; d++) {
            const uint32_t node = aoh_path_node(d, prefix), ctx = hist & mask;
            if (snap_ctx[node] != ctx) rc = -1;
            const uint32_t cv = variant == 2 ? snap[node] : aoh_forward(nb, d, ctx, snap[node]);
            const uint32_t bit = w3o_ac_decode(&ac, (uint16_t)counter_p(cv), &rd);
            nb.ctx[d] = ctx; nb.upd[d] = counter_update(cv, bit);
            hist = (hist << 1) | bit;
            prefix = (prefix << 1) | bit;
            if (left) {   // the job ends on its byte count: the nibble's later steps are discarded
                n_steps = d + 1;
                uint32_t sym;
                if (aoh_walk(walk, bit, t.fc, t.offs, t.sym, t.max_len, sym)) {
                    left--;
                    uint32_t word;
                    const uint32_t nst = aoh_out_put(ob, sym, (uint32_t)(uintptr_t)(out + i), left == 0, word);
                    i++;
                    if (nst == 4) {
                        if ((uintptr_t)(out + i - 4) & 3u) rc = -2;   // a word store must be aligned
                        memcpy(out + i - 4, &word, 4);
                        (*word_stores)++;
                    } else for (uint32_t k = 0; k < nst; k++) out[i - nst + k] = (uint8_t)(word >> (8 * k));
                }
            }
        }
        for (uint32_t d = n_steps; d-- > 0;)
            if (variant == 1 || aoh_last_writer(nb, d, n_steps)) table[nb.ctx[d]] = nb.upd[d];
        counts[0]++;
        if (n_steps == 4) {
            counts[1]++;
            bool eq = false;
            for (uint32_t d = 0; d < 4; d++)
                for (uint32_t e = d + 1; e < 4; e++) eq |= nb.ctx[d] == nb.ctx[e];
            counts[2] += eq;
        }
    }
    free(table);
    return rc;
}
