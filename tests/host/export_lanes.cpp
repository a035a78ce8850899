// Host harness for weath3rb0i_amd/csrc/w3_export.h (tests/test_export_cpu.py, tests/test_gpu_export.py): the context statistics export
// the way the kernels compute it — count, apply and replay per epoch, the 64 "lanes" of a wavefront as loops (WaveHost) — compiled for
// the CPU, and the yardstick it is compared with HERE: a literal restatement of ordern.rs:26-44 and counter.rs:20-26 (history, alignment
// and ctx updated step by step, Counter::update per step), which never calls the code under test.
//   export_lanes <blob file> <case file>      one case per line, one answer line per case: "ok ..." or "BAD ..."
//     exp <input> <bits> <align> <E> <a> [cuts..]   the device form of <input> under OrderN(bits, align) with epochs of E bytes (0: the
//                     length rounded up to whole KiB) against the literal replay.  a = 0 .. 15: the buffer a bytes past a 16-byte
//                     boundary in a heap block that ends with it; 16: starting at a page start behind an inaccessible page; 17: ending at
//                     a page end before one.  cuts: the stream as several pieces cut at those byte offsets (each piece in a buffer of
//                     its own, epochs starting anew in every piece, history bits and offset carried).  bits <= 24.
//     lit <input> <bits> <align> <E> <out file>     the literal replay alone (bits <= 28): the nonzero entries to <out file> as pairs
//                     of uint32 (ctx, n0 | n1 << 16), ascending
//   <input>: blob:<off>:<len> | ffz:<p>:<len> (p bytes 0xFF, then len zero bytes)   (lanes_common.h)
//   answers: "ok replays=<listed (context, epoch) pairs> halvings=<n> epochs=<n> nonzero=<entries> fold=<FNV-1a of the table>"
#include <sstream>
#include <unordered_map>

#define W3_HD static inline
#include "../../weath3rb0i_amd/csrc/w3_export.h"
#define LANES_EXPORT_FORM   // (Form: the device form of a piece over w3_export.h, included above)
#include "lanes_common.h"

// ---- the yardstick: OrderN + Counter, literally ---------------------------------------------------------------------------------------
struct OrderN {
    std::vector<Counter> dense;
    std::unordered_map<uint32_t, Counter> sparse;   // tables above 2^26 contexts
    uint32_t ctx = 0, history = 0;
    uint8_t alignment = 0, bits_in_context, alignment_bits;
    OrderN(uint8_t bits, uint8_t align) : bits_in_context(bits), alignment_bits(align) {
        if (bits <= 26) dense.resize((size_t)1 << bits);
    }
    Counter &at(uint32_t c) { return dense.empty() ? sparse[c] : dense[c]; }
    bool adapt(uint8_t bit) { return at(ctx).update(bit); }   // ordern.rs:30-32
    void update(uint8_t bit) {                                // ordern.rs:34-43
        const uint32_t mask_bits = (uint32_t)bits_in_context - alignment_bits;
        const uint32_t mask = (uint32_t)((1ull << mask_bits) - 1);
        const uint8_t alignment_mask = (uint8_t)((1u << alignment_bits) - 1);
        history = ((history << 1) | bit) & mask;
        alignment = (uint8_t)((alignment + 1) & alignment_mask);
        ctx = (history << alignment_bits) | alignment;
    }
    void feed(const uint8_t *buf, size_t n, uint64_t byte0, std::vector<Halving> &where) {
        for (size_t k = 0; k < n; k++)
            for (int j = 7; j >= 0; j--) {
                const uint8_t bit = (buf[k] >> j) & 1;
                if (adapt(bit)) where.push_back({byte0 + k, ctx});
                update(bit);
            }
    }
    uint32_t packed(uint32_t c) { const Counter &x = at(c); return (uint32_t)x.data[0] | ((uint32_t)x.data[1] << 16); }
};

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: export_lanes <blob> <cases>\n"); return 2; }
    std::vector<uint8_t> blob;
    if (!load_blob(argv[1], blob)) return 2;
    FILE *cf = fopen(argv[2], "r");
    if (!cf) { perror(argv[2]); return 2; }
    static char line[1 << 16];
    while (fgets(line, sizeof line, cf)) {
        std::istringstream in(line);
        std::string kind, ispec;
        unsigned bits = 0, align = 0;
        unsigned long long E = 0;
        in >> kind >> ispec >> bits >> align >> E;
        std::vector<uint8_t> data;
        if (!in || !make_input(blob, ispec, data) || bits < 1 || align > 7 || align > bits || (kind != "exp" && kind != "lit")) { fprintf(stderr, "bad case: %s", line); return 2; }
        const uint64_t n = data.size();
        if (E == 0) E = std::max<uint64_t>((n + 1023) / 1024 * 1024, 1024);
        if (E % 1024) { fprintf(stderr, "bad epoch: %s", line); return 2; }
        OrderN lit((uint8_t)bits, (uint8_t)align);
        std::vector<Halving> where;
        lit.feed(data.data(), (size_t)n, 0, where);
        std::string r;
        char buf[256];
        if (kind == "lit") {
            std::string path;
            in >> path;
            if (!in || bits > 28) { fprintf(stderr, "bad case: %s", line); return 2; }
            std::vector<uint32_t> keys;
            if (lit.dense.empty()) { for (auto &kv : lit.sparse) keys.push_back(kv.first); }
            else { for (uint32_t c = 0; c < lit.dense.size(); c++) if (lit.packed(c)) keys.push_back(c); }
            std::sort(keys.begin(), keys.end());
            FILE *o = fopen(path.c_str(), "wb");
            if (!o) { perror(path.c_str()); return 2; }
            uint64_t nonzero = 0, fold = FNV0;
            for (uint32_t c : keys) {
                const uint32_t pair[2] = {c, lit.packed(c)};
                if (!pair[1]) continue;
                fwrite(pair, 4, 2, o);
                nonzero++;
                fold = fnv(fnv(fold, pair[0]), pair[1]);
            }
            fclose(o);
            const uint64_t pairs = literal_pairs(where, pieces_of(n, {}), E);
            snprintf(buf, sizeof buf, "ok replays=%llu halvings=%llu epochs=%llu nonzero=%llu fold=%016llx", (unsigned long long)pairs,
                     (unsigned long long)where.size(), (unsigned long long)((n + E - 1) / E), (unsigned long long)nonzero, (unsigned long long)fold);
            r = buf;
        } else {
            unsigned a = 0;
            in >> a;
            if (!in || a > 17 || bits > 24) { fprintf(stderr, "bad case: %s", line); return 2; }
            std::vector<uint64_t> cuts;
            unsigned long long x;
            while (in >> x) cuts.push_back(x);
            const auto pieces = pieces_of(n, cuts);
            Form f(bits, align);   // the device form (lanes_common.h) over the raw source
            uint64_t carry = 0;
            for (const auto &pr : pieces)
                in_buffer(data.data() + pr.first, (size_t)(pr.second - pr.first), a, [&](const uint8_t *p) {
                    const w3::ExpPiece pc = {p, pr.second - pr.first, pr.first, carry, 0u};
                    f.piece(pc, E, [&](uint64_t e0, uint64_t len) { return w3::ExpRawSrc{pc, e0, len, f.m}; });
                    carry = w3::exp_window(pc, pc.n);
                });
            uint64_t nonzero = 0, fold = FNV0;
            for (uint32_t c = 0; c < f.S.size(); c++)
                if (lit.packed(c)) { nonzero++; fold = fnv(fnv(fold, c), lit.packed(c)); }
            r = f.verdict([&](uint32_t c) { return lit.packed(c); }, literal_pairs(where, pieces, E), where.size(), n);
            if (r.empty()) {
                snprintf(buf, sizeof buf, "ok replays=%llu halvings=%llu epochs=%llu nonzero=%llu fold=%016llx", (unsigned long long)f.replays,
                         (unsigned long long)f.halvings, (unsigned long long)f.epochs, (unsigned long long)nonzero, (unsigned long long)fold);
                r = buf;
            }
        }
        puts(r.c_str());
        fflush(stdout);
    }
    fclose(cf);
    return 0;
}
