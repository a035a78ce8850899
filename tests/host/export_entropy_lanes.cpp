// Host harness for weath3rb0i_amd/csrc/w3_export_entropy.h (tests/test_export_entropy_cpu.py, tests/test_gpu_export_entropy.py): the
// context statistics export for OrderNEntropy leaves the way the kernels compute it — a key stage per epoch, keyed count, apply and
// keyed replay, the 64 "lanes" of a wavefront as loops (WaveHost) — compiled for the CPU, and the yardstick it is compared with HERE: a
// literal restatement of ordern_entropy.rs:27-45 and counter.rs:20-26 (Counter::update per adapt; history.update, alignment, hash and ctx
// per step) with History::update / hash taken from the oracle (oracle/w3_oracle.c: w3o_history_*), which never calls the code under test.
// Built as a stand-alone program:  gcc -c oracle/w3_oracle.c;  g++ -I oracle tests/host/export_entropy_lanes.cpp w3_oracle.o
//   export_entropy_lanes <blob file> <case file>      one case per line, one answer line per case: "ok ..." or "BAD ..."
//     exp <input> <history> <bits> <align> <E> <a> [cuts..]   the device form of <input> under OrderNEntropy(bits, align, <history>) with
//                     epochs of E bytes (0: the length rounded up to whole KiB) against the literal run: the keys of every epoch, the
//                     table, D left zeroed, replays, halvings.  a = 0 .. 15: the buffer a bytes past a 16-byte boundary in a heap block
//                     that ends with it; 16: starting at a page start behind an inaccessible page; 17: ending at a page end before one.
//                     cuts: the stream as several pieces cut at those byte offsets (each piece in a buffer of its own, epochs starting
//                     anew in every piece; the 8-byte carry, the offset and the Huffman seed carried as the staged call carries them).
//     lit <input> <history> <bits> <align> <E> <out file>     the literal run alone: the nonzero entries to <out file> as pairs of uint32
//                     (ctx, n0 | n1 << 16), ascending
//   <input>: blob:<off>:<len> | ffz:<p>:<len> (p bytes 0xFF, then len zero bytes) | zrun:<a>:<z>:<f>:<b> (blob[0:a], z zero bytes, f bytes
//            0xFF, blob[a:a+b])
//   <history>: ac:<max_bits>:book1 | ac:<max_bits>:new (StationaryModel::new on the input) | huff:<huff_size>:<rem_huff_size>:<len>
//            (HuffHistory::new on blob[0:len])
//   answers: "ok replays=<listed (context, epoch) pairs> halvings=<n> epochs=<n> nonzero=<entries> halvctx=<contexts that halve>
//            fixed=<epochs redone by the recurrence> len0=<len[0]> len255=<len[255]> e0=<entry 0> e2040=<entry 2040> fold=<FNV-1a of the
//            table> hbytes=<the distinct bytes on which the literal run halves, comma separated, or ->"
// The AC key stage here takes ACHistory::hash of a window from the oracle: ac_history_hash_steps (w3_device.h) is written over wavefront
// ballots and device intrinsics and is covered on the GPU only.  The window (across epochs, pieces and the carry), the key's composition
// and everything behind the keys are the header's own code.
#include <map>
#include <memory>
#include <sstream>

extern "C" {
#include "w3_oracle.h"
}

#define W3_HD static inline
#include "../../weath3rb0i_amd/csrc/w3_export_entropy.h"
#define LANES_EXPORT_FORM   // (Form: the device form of a piece over w3_export.h, included above)
#include "lanes_common.h"

// ---- the yardstick: OrderNEntropy + Counter, literally ----------------------------------------------------------------------------------
struct Literal {
    std::vector<Counter> stats;
    std::vector<uint32_t> keys;   // ctx | bit << 31 of every step: what the key stage has to produce
    std::vector<Halving> where;
    Literal(const uint8_t *buf, size_t n, uint8_t bits_in_context, uint8_t alignment_bits, w3o_history history) : stats((size_t)1 << bits_in_context) {
        uint32_t ctx = 0;            // ordern_entropy.rs:15-24
        uint8_t alignment = 0;
        keys.reserve(n * 8);
        for (size_t k = 0; k < n; k++)
            for (int j = 7; j >= 0; j--) {
                const uint8_t bit = (buf[k] >> j) & 1;
                keys.push_back(ctx | ((uint32_t)bit << 31));
                if (stats[ctx].update(bit)) where.push_back({k, ctx});   // adapt  :32-34
                const uint32_t mask_bits = (uint32_t)bits_in_context - alignment_bits;   // update  :36-45
                const uint32_t mask = (uint32_t)((1ull << mask_bits) - 1);
                const uint8_t alignment_mask = (uint8_t)((1u << alignment_bits) - 1);
                w3o_history_update(&history, bit);
                alignment = (uint8_t)((alignment + 1) & alignment_mask);
                const uint32_t hash = w3o_history_hash(&history) & mask;
                ctx = (hash << alignment_bits) | alignment;
            }
    }
    uint32_t packed(uint32_t c) const { return (uint32_t)stats[c].data[0] | ((uint32_t)stats[c].data[1] << 16); }
};

// ---- the device form --------------------------------------------------------------------------------------------------------------------
struct AlignedKeys {   // a heap block of exactly `steps` keys, 16-byte aligned: a load behind the last step is the sanitizer's
    uint32_t *p = nullptr;
    explicit AlignedKeys(uint64_t steps) {
        if (posix_memalign((void **)&p, 16, steps ? (size_t)steps * 4 : 16)) abort();
        memset(p, 0xA5, steps ? (size_t)steps * 4 : 16);
    }
    ~AlignedKeys() { free(p); }
    AlignedKeys(const AlignedKeys &) = delete;
};
// the key stage of one epoch as the kernels run it, compared with the literal run's keys: what KeyedForm::piece hands to Form::piece
struct KeyedForm : Form {
    w3o_history hist;   // kind, max_bits, model, huff: the leaf's parameters
    uint64_t fixed = 0;
    KeyedForm(uint32_t bits, uint32_t align, const w3o_history &h) : Form(bits, align), hist(h) {}
    uint32_t ac_hash(uint64_t window, uint32_t j) {   // ACHistory::hash of the oracle with this history
        w3o_history h = hist;
        h.bits = window; h.pos = j;
        return w3o_history_hash(&h);
    }
    void piece(const w3::ExpPiece &pc, uint64_t E, const std::vector<uint32_t> &want_keys) {
        bool chained = false;   // W3_EXPK_HS_* of the device, zeroed per piece
        uint32_t chain_cb = 0;
        std::unique_ptr<AlignedKeys> keys;   // (the epoch's: freed when the next epoch's are made)
        Form::piece(pc, E, [&](uint64_t e0, uint64_t len) {
            const uint64_t steps = len * 8;
            keys.reset(new AlignedKeys(steps));
            uint32_t *K = keys->p;
            if (hist.kind == W3O_HIST_AC) {   // k_expk_ackeys
                for (uint64_t g = 0; g < steps; g++) {
                    const uint64_t i = e0 + (g >> 3);
                    const uint32_t j = (uint32_t)g & 7u, c0 = pc.p[i];
                    const uint64_t h64 = (w3::exp_window(pc, i) << j) | (uint64_t)(c0 >> (8u - j));
                    K[g] = w3::expk_key(m, ac_hash(h64, j), (pc.abs0 + i) * 8u + j, (c0 >> (7u - j)) & 1u);
                }
            } else {   // k_expk_huffkeys, k_expk_huff_fix
                const w3o_huff_tables &t = hist.huff;
                bool flagged = false;
                for (uint64_t g = 0; g < len; g++) {
                    uint32_t k[8];
                    if (!w3::expk_huff_byte(pc, e0, g, m, t.code, t.len, t.rem_code, t.rem_len, k)) flagged = true;
                    memcpy(K + 8 * g, k, 32);
                }
                if (flagged) {
                    const uint32_t seed = w3::expk_huff_epoch_seed(pc, e0, chained, chain_cb, t.code, t.len);
                    chain_cb = w3::expk_huff_redo(pc, e0, len, m, seed, t.code, t.len, t.rem_code, t.rem_len, K);
                    fixed++;
                }
                chained = flagged;
            }
            const uint32_t *want = want_keys.data() + (pc.abs0 + e0) * 8;
            if (bad.empty() && memcmp(K, want, (size_t)steps * 4)) {
                uint64_t g = 0;
                while (K[g] == want[g]) g++;
                char buf[160];
                snprintf(buf, sizeof buf, "key of stream step %llu: %08x, the literal run has %08x", (unsigned long long)((pc.abs0 + e0) * 8 + g), K[g], want[g]);
                bad = buf;
            }
            return w3::ExpKeySrc{K, steps};
        });
    }
};

static bool make_history(const std::vector<uint8_t> &blob, const std::string &spec, const std::vector<uint8_t> &data, w3o_history &h) {
    unsigned a = 0, b = 0;
    unsigned long long len = 0;
    char name[16] = {0};
    if (sscanf(spec.c_str(), "ac:%u:%15s", &a, name) == 2 && a <= 32) {
        w3o_stationary m;
        if (!strcmp(name, "book1")) w3o_stationary_for_book1(&m);
        else if (!strcmp(name, "new")) w3o_stationary_new(&m, data.data(), data.size());
        else return false;
        w3o_history_ac(&h, (uint8_t)a, &m);
        return true;
    }
    if (sscanf(spec.c_str(), "huff:%u:%u:%llu", &a, &b, &len) == 3 && len <= blob.size()) {
        w3o_huff_tables t;
        if (w3o_huff_tables_new(blob.data(), (size_t)len, (uint8_t)a, (uint8_t)b, &t)) return false;
        w3o_history_huff(&h, &t);
        return true;
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: export_entropy_lanes <blob> <cases>\n"); return 2; }
    std::vector<uint8_t> blob;
    if (!load_blob(argv[1], blob)) return 2;
    FILE *cf = fopen(argv[2], "r");
    if (!cf) { perror(argv[2]); return 2; }
    std::map<std::string, std::shared_ptr<Literal>> literals;   // by input, history and shape: the cases of one file share them
    static char line[1 << 16];
    while (fgets(line, sizeof line, cf)) {
        std::istringstream in(line);
        std::string kind, ispec, hspec;
        unsigned bits = 0, align = 0;
        unsigned long long E = 0;
        in >> kind >> ispec >> hspec >> bits >> align >> E;
        std::vector<uint8_t> data;
        w3o_history hist;
        if (!in || !make_input(blob, ispec, data) || !make_history(blob, hspec, data, hist) || bits < 1 || bits > 24 || align > 7 || align > bits ||
            (kind != "exp" && kind != "lit")) { fprintf(stderr, "bad case: %s", line); return 2; }
        const uint64_t n = data.size();
        if (E == 0) E = std::max<uint64_t>((n + 1023) / 1024 * 1024, 1024);
        if (E % 1024) { fprintf(stderr, "bad epoch: %s", line); return 2; }
        char lkey[256];
        snprintf(lkey, sizeof lkey, "%s %s %u %u", ispec.c_str(), hspec.c_str(), bits, align);
        std::shared_ptr<Literal> &slot = literals[lkey];
        if (!slot) slot = std::make_shared<Literal>(data.data(), (size_t)n, (uint8_t)bits, (uint8_t)align, hist);
        const Literal &lit = *slot;
        std::set<uint32_t> halvctx;
        std::set<uint64_t> hbytes;
        for (const Halving &h : lit.where) { halvctx.insert(h.ctx); hbytes.insert(h.byte); }
        std::string hb;
        for (uint64_t b : hbytes) hb += (hb.empty() ? "" : ",") + std::to_string(b);
        if (hb.empty()) hb = "-";
        uint64_t nonzero = 0, fold = FNV0;
        for (uint32_t c = 0; c < lit.stats.size(); c++)
            if (lit.packed(c)) { nonzero++; fold = fnv(fnv(fold, c), lit.packed(c)); }
        const unsigned len0 = hist.kind == W3O_HIST_HUFF ? hist.huff.len[0] : 99, len255 = hist.kind == W3O_HIST_HUFF ? hist.huff.len[255] : 99;
        const uint32_t e2040 = lit.stats.size() > 2040 ? lit.packed(2040) : 0;
        std::string r;
        char buf[512];
        uint64_t replays = 0, halvings = lit.where.size(), epochs = (n + E - 1) / E, fixed = 0;
        if (kind == "lit") {
            std::string path;
            in >> path;
            if (!in) { fprintf(stderr, "bad case: %s", line); return 2; }
            FILE *o = fopen(path.c_str(), "wb");
            if (!o) { perror(path.c_str()); return 2; }
            for (uint32_t c = 0; c < lit.stats.size(); c++) {
                const uint32_t pair[2] = {c, lit.packed(c)};
                if (pair[1]) fwrite(pair, 4, 2, o);
            }
            fclose(o);
            replays = literal_pairs(lit.where, pieces_of(n, {}), E);
        } else {
            unsigned a = 0;
            in >> a;
            if (!in || a > 17) { fprintf(stderr, "bad case: %s", line); return 2; }
            std::vector<uint64_t> cuts;
            unsigned long long x;
            while (in >> x) cuts.push_back(x);
            const auto pieces = pieces_of(n, cuts);
            KeyedForm f(bits, align, hist);
            uint64_t carry = 0, prev = 0;
            uint32_t seed = 0;
            for (const auto &pr : pieces) {
                if (hist.kind == W3O_HIST_HUFF && pr.first) seed = w3::expk_huff_piece_seed(data.data(), pr.first, prev, seed, hist.huff.code, hist.huff.len);
                prev = pr.first;
                in_buffer(data.data() + pr.first, (size_t)(pr.second - pr.first), a, [&](const uint8_t *p) {
                    const w3::ExpPiece pc = {p, pr.second - pr.first, pr.first, carry, seed};
                    f.piece(pc, E, lit.keys);
                    carry = w3::exp_window(pc, pc.n);
                });
            }
            r = f.verdict([&](uint32_t c) { return lit.packed(c); }, literal_pairs(lit.where, pieces, E), lit.where.size(), n);
            replays = f.replays; epochs = f.epochs; fixed = f.fixed;
        }
        if (r.empty()) {
            snprintf(buf, sizeof buf, "ok replays=%llu halvings=%llu epochs=%llu nonzero=%llu halvctx=%llu fixed=%llu len0=%u len255=%u e0=%u e2040=%u fold=%016llx hbytes=",
                     (unsigned long long)replays, (unsigned long long)halvings, (unsigned long long)epochs, (unsigned long long)nonzero,
                     (unsigned long long)halvctx.size(), (unsigned long long)fixed, len0, len255, lit.stats.empty() ? 0u : lit.packed(0), e2040,
                     (unsigned long long)fold);
            r = buf + hb;
        }
        puts(r.c_str());
        fflush(stdout);
    }
    fclose(cf);
    return 0;
}
