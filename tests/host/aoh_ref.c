/* CPU truth of the AC-over-Huffman coder for the tests: the loop of bin/ac-over-huffman/main.rs:69-89 composed from the oracle's own
 * parts (w3o_ordern, w3o_ac_*, the byte and counting sinks), on the block container, over threads.  A C restatement, not the
 * reference.  Built on demand by tests/aoh_ref.py:  gcc -O2 -shared -fPIC -I oracle tests/host/aoh_ref.c oracle/w3_oracle.c -lpthread -lm
 *   block b: fresh OrderN(ctx_bits, 0) and coder; for every byte, its code's bits MSB first:
 *            p = predict(); update(bit); encode(bit, p)   (:81-84);  flush (:87).
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "w3_oracle.h"

typedef struct {
    const uint16_t *code; const uint8_t *len; uint8_t ctx_bits;
    const uint8_t *in; size_t n, block_size, nblocks;
    int mode;                    /* 0 = streams, 1 = ACStats bit counts, 2 = decode */
    uint8_t **streams; size_t *stream_len;   /* mode 0: per block, malloc'ed */
    uint64_t *bits;                          /* mode 1 */
    const uint8_t *cin; const uint64_t *coffs; const uint32_t *clens; uint8_t *dout;   /* mode 2 */
    size_t first, step;
} aoh_job;

static void code_block(const aoh_job *j, w3o_model *m, size_t b) {
    const size_t off = b * j->block_size, len = j->n - off < j->block_size ? j->n - off : j->block_size;
    w3o_model_reset(m);
    if (j->mode == 2) {
        /* decode tables: symbols by (len, code); a prefix of length l is a symbol when some symbol has that (code, len) */
        w3o_reader r; w3o_ac ac;
        w3o_reader_init(&r, j->cin + j->coffs[b], j->clens[b]);
        w3o_ac_new_decoder(&ac, &r);
        for (size_t i = 0; i < len; i++) {
            uint32_t code = 0; unsigned l = 0; int sym = -1;
            while (sym < 0 && l < 16) {
                const uint16_t p = w3o_model_predict(m);
                const uint8_t bit = w3o_ac_decode(&ac, p, &r);
                w3o_model_update(m, bit);
                code = code << 1 | bit; l++;
                for (int s = 0; s < 256; s++) if (j->len[s] == l && j->code[s] == code) { sym = s; break; }
            }
            j->dout[off + i] = (uint8_t)(sym < 0 ? 0 : sym);
        }
        return;
    }
    w3o_sink w; w3o_ac ac;
    if (j->mode == 0) w3o_sink_init_bytes(&w); else w3o_sink_init_stats(&w);
    w3o_ac_new_coder(&ac);
    for (size_t i = 0; i < len; i++) {
        const uint16_t code = j->code[j->in[off + i]];
        for (int k = (int)j->len[j->in[off + i]] - 1; k >= 0; k--) {
            const uint16_t p = w3o_model_predict(m);
            const uint8_t bit = (uint8_t)((code >> k) & 1);
            w3o_model_update(m, bit);
            w3o_ac_encode(&ac, bit, p, &w);
        }
    }
    if (j->mode == 1) j->bits[b] = w.bit_count;   /* the raw count; csize = bits / 8 (helpers.rs:70-73); flush adds nothing (:87-89) */
    w3o_ac_flush(&ac, &w);
    if (j->mode == 0) { j->streams[b] = w.buf; j->stream_len[b] = w.len; }
    else w3o_sink_free(&w);
}

static void *worker(void *arg) {
    const aoh_job *j = (const aoh_job *)arg;
    w3o_model *m = w3o_ordern(j->ctx_bits, 0);
    for (size_t b = j->first; b < j->nblocks; b += j->step) code_block(j, m, b);
    w3o_model_free(m);
    return NULL;
}

static void run(aoh_job *proto, int nthreads) {
    if (nthreads < 1) nthreads = 1;
    if (proto->ctx_bits > 27 && nthreads > 4) nthreads = 4;   /* (a model of 2^ctx_bits Counters per thread: 8 GiB of address space at 31) */
    if ((size_t)nthreads > proto->nblocks) nthreads = (int)(proto->nblocks ? proto->nblocks : 1);
    pthread_t *th = (pthread_t *)malloc(sizeof(pthread_t) * (size_t)nthreads);
    aoh_job *jobs = (aoh_job *)malloc(sizeof(aoh_job) * (size_t)nthreads);
    for (int t = 0; t < nthreads; t++) { jobs[t] = *proto; jobs[t].first = (size_t)t; jobs[t].step = (size_t)nthreads; pthread_create(&th[t], NULL, worker, &jobs[t]); }
    for (int t = 0; t < nthreads; t++) pthread_join(th[t], NULL);
    free(th); free(jobs);
}

/* streams concatenated into out (cap out_cap), block_lens[nblocks]; returns 0, or -2 with *out_len = the size needed */
int aoh_encode_blocks(const uint16_t *code, const uint8_t *len, uint8_t ctx_bits, const uint8_t *in, size_t n, size_t block_size,
                      uint8_t *out, size_t out_cap, size_t *out_len, uint32_t *block_lens, int nthreads) {
    aoh_job j; memset(&j, 0, sizeof j);
    j.code = code; j.len = len; j.ctx_bits = ctx_bits; j.in = in; j.n = n; j.block_size = block_size;
    j.nblocks = (n + block_size - 1) / block_size; j.mode = 0;
    j.streams = (uint8_t **)calloc(j.nblocks ? j.nblocks : 1, sizeof(uint8_t *));
    j.stream_len = (size_t *)calloc(j.nblocks ? j.nblocks : 1, sizeof(size_t));
    run(&j, nthreads);
    size_t total = 0;
    for (size_t b = 0; b < j.nblocks; b++) total += j.stream_len[b];
    *out_len = total;
    size_t o = 0;
    for (size_t b = 0; b < j.nblocks; b++) {
        if (total <= out_cap) memcpy(out + o, j.streams[b], j.stream_len[b]);
        block_lens[b] = (uint32_t)j.stream_len[b];
        o += j.stream_len[b];
        free(j.streams[b]);
    }
    free(j.streams); free(j.stream_len);
    return total <= out_cap ? 0 : -2;
}

void aoh_stats_bits(const uint16_t *code, const uint8_t *len, uint8_t ctx_bits, const uint8_t *in, size_t n, size_t block_size,
                    uint64_t *block_bits, int nthreads) {
    aoh_job j; memset(&j, 0, sizeof j);
    j.code = code; j.len = len; j.ctx_bits = ctx_bits; j.in = in; j.n = n; j.block_size = block_size;
    j.nblocks = (n + block_size - 1) / block_size; j.mode = 1; j.bits = block_bits;
    run(&j, nthreads);
}

void aoh_decode_blocks(const uint16_t *code, const uint8_t *len, uint8_t ctx_bits, const uint8_t *cin, const uint32_t *block_lens,
                       size_t block_size, size_t orig_len, uint8_t *out, int nthreads) {
    aoh_job j; memset(&j, 0, sizeof j);
    j.code = code; j.len = len; j.ctx_bits = ctx_bits; j.n = orig_len; j.block_size = block_size;
    j.nblocks = (orig_len + block_size - 1) / block_size; j.mode = 2;
    uint64_t *coffs = (uint64_t *)calloc(j.nblocks ? j.nblocks : 1, sizeof(uint64_t));
    uint64_t o = 0;
    for (size_t b = 0; b < j.nblocks; b++) { coffs[b] = o; o += block_lens[b]; }
    j.cin = cin; j.coffs = coffs; j.clens = block_lens; j.dout = out;
    run(&j, nthreads);
    free(coffs);
}
