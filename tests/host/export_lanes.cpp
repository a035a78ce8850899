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
//   <input>: blob:<off>:<len> | ffz:<p>:<len> (p bytes 0xFF, then len zero bytes)
//   answers: "ok replays=<listed (context, epoch) pairs> halvings=<n> epochs=<n> nonzero=<entries> fold=<FNV-1a of the table>"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <sstream>
#include <string>
#include <sys/mman.h>
#include <unistd.h>
#include <unordered_map>
#include <vector>

#define W3_HD static inline
#include "../../weath3rb0i_amd/csrc/w3_export.h"

// ---- the yardstick: OrderN + Counter, literally ---------------------------------------------------------------------------------------
struct Counter {
    uint16_t data[2] = {0, 0};
    bool update(uint8_t bit) {   // counter.rs:20-26; true if it halved
        data[bit] += 1;
        if (data[bit] == 0xFFFF) {
            data[0] = (uint16_t)((data[0] >> 1) + (data[0] & 1));
            data[1] = (uint16_t)((data[1] >> 1) + (data[1] & 1));
            return true;
        }
        return false;
    }
};
struct Halving { uint64_t byte; uint32_t ctx; };
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

// ---- the device form --------------------------------------------------------------------------------------------------------------------
struct Form {
    w3::ExpModel m;
    std::vector<uint64_t> D;
    std::vector<uint32_t> S;
    uint64_t replays = 0, halvings = 0, epochs = 0;
    std::string bad;
    Form(uint32_t bits, uint32_t align) : m{bits, align}, D((size_t)1 << bits), S((size_t)1 << bits) {}
    // one piece, as a device call runs it: per epoch k_ctx_count (here: 7 waves striding over the rows), k_ctx_apply, k_ctx_replay
    void piece(const w3::ExpPiece &pc, uint64_t E) {
        std::vector<uint32_t> touched, list;
        for (uint64_t e0 = 0; e0 < pc.n; e0 += E) {
            const uint64_t len = std::min<uint64_t>(E, pc.n - e0);
            const uint64_t nw = 7;
            touched.clear();
            for (uint64_t gw = 0; gw < nw; gw++)
                for (uint32_t lane = 0; lane < 64; lane++)
                    w3::exp_count_wave_lane(pc, e0, len, m, lane, gw, nw, [&](uint32_t ctx, uint32_t bit) {
                        if (!D[ctx]) touched.push_back(ctx);
                        D[ctx] += bit ? 1ull << 32 : 1ull;
                    });
            list.clear();
            for (uint32_t c : touched) {   // (k_ctx_apply visits every context and skips D == 0)
                if (w3::exp_apply(D[c], S[c])) list.push_back(c);
                D[c] = 0;
            }
            if (list.size() > w3::exp_list_cap(m.bits, pc.abs0 + e0 + len)) bad = "the replay list exceeds its bound";
            w3::WaveHost wv;
            for (uint32_t c : list) {
                const uint32_t h = w3::exp_replay(wv, pc, e0, len, m, c, S[c]);
                if (!h) bad = "a listed context without a halving";
                halvings += h;
            }
            replays += list.size();
            epochs++;
        }
    }
};

struct Heap {   // a heap block that ENDS with the data, a bytes past a 16-byte boundary, other values before it
    uint8_t *raw = nullptr, *p = nullptr;
    Heap(size_t n, unsigned a) {
        if (posix_memalign((void **)&raw, 16, a + n ? a + n : 1)) abort();
        memset(raw, 0xA5, a);
        p = raw + a;
    }
    ~Heap() { free(raw); }
    Heap(const Heap &) = delete;
};
struct Guarded {   // [p, p + n) starting at a page start behind an inaccessible page (end = false) or ending at a page end before one
    uint8_t *m = nullptr, *p = nullptr;
    size_t total = 0;
    Guarded(size_t n, bool end) {
        const size_t page = (size_t)sysconf(_SC_PAGESIZE), pages = (n + page - 1) / page + 1;
        total = (pages + 2) * page;
        m = (uint8_t *)mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) { perror("mmap"); exit(2); }
        memset(m + page, 0xA5, pages * page);
        if (mprotect(m, page, PROT_NONE) || mprotect(m + (pages + 1) * page, page, PROT_NONE)) { perror("mprotect"); exit(2); }
        p = end ? m + (pages + 1) * page - n : m + page;
    }
    ~Guarded() { munmap(m, total); }
    Guarded(const Guarded &) = delete;
};

static std::vector<uint8_t> blob;

static bool make_input(const std::string &spec, std::vector<uint8_t> &out) {
    unsigned long long a = 0, b = 0;
    if (sscanf(spec.c_str(), "blob:%llu:%llu", &a, &b) == 2) {
        if (a + b > blob.size()) return false;
        out.assign(blob.begin() + (long)a, blob.begin() + (long)(a + b));
        return true;
    }
    if (sscanf(spec.c_str(), "ffz:%llu:%llu", &a, &b) == 2) {
        out.assign((size_t)(a + b), 0);
        std::fill(out.begin(), out.begin() + (long)a, 0xFF);
        return true;
    }
    return false;
}

static uint64_t fnv(uint64_t h, uint64_t v) { return (h ^ v) * 1099511628211ull; }

// the pieces [lo, hi) the cut list makes of n bytes
static std::vector<std::pair<uint64_t, uint64_t>> pieces_of(uint64_t n, const std::vector<uint64_t> &cuts) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    uint64_t lo = 0;
    for (size_t k = 0; k <= cuts.size(); k++) {
        const uint64_t hi = k < cuts.size() ? std::min(cuts[k], n) : n;
        if (hi < lo) continue;
        if (hi > lo || (n == 0 && k == cuts.size())) out.push_back({lo, hi});
        lo = hi;
    }
    return out;
}

// (context, epoch) pairs in which the literal replay halves, for pieces cut as above with epochs of E bytes from every piece's start
static uint64_t literal_pairs(const std::vector<Halving> &where, const std::vector<std::pair<uint64_t, uint64_t>> &pieces, uint64_t E) {
    std::set<std::pair<uint64_t, uint32_t>> pairs;
    for (const Halving &h : where) {
        uint64_t id = 0;
        for (const auto &pc : pieces) {
            if (h.byte >= pc.first && h.byte < pc.second) { id += (h.byte - pc.first) / E; break; }
            id += (pc.second - pc.first + E - 1) / E;
        }
        pairs.insert({id, h.ctx});
    }
    return pairs.size();
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: export_lanes <blob> <cases>\n"); return 2; }
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        blob.resize((size_t)n);
        if (n && fread(blob.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
        fclose(f);
    }
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
        if (!in || !make_input(ispec, data) || bits < 1 || align > 7 || align > bits || (kind != "exp" && kind != "lit")) { fprintf(stderr, "bad case: %s", line); return 2; }
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
            uint64_t nonzero = 0, fold = 1469598103934665603ull;
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
            Form f(bits, align);
            uint32_t carry = 0;
            for (const auto &pr : pieces) {
                const uint64_t len = pr.second - pr.first;
                w3::ExpPiece pc;
                pc.n = len; pc.abs0 = pr.first; pc.carry = carry;
                if (a <= 15) {
                    Heap h((size_t)len, a);
                    if (len) memcpy(h.p, data.data() + pr.first, (size_t)len);
                    pc.p = h.p;
                    f.piece(pc, E);
                    carry = w3::exp_hist_before(pc, len);
                } else {
                    Guarded g((size_t)len, a == 17);
                    if (len) memcpy(g.p, data.data() + pr.first, (size_t)len);
                    pc.p = g.p;
                    f.piece(pc, E);
                    carry = w3::exp_hist_before(pc, len);
                }
            }
            const uint64_t pairs = literal_pairs(where, pieces, E);
            uint64_t nonzero = 0, fold = 1469598103934665603ull, diff = 0, first = 0;
            for (uint32_t c = 0; c < f.S.size(); c++) {
                const uint32_t want = lit.packed(c);
                if (f.S[c] != want && !diff++) first = c;
                if (f.D[c]) f.bad = "D is not left zeroed";
                if (want) { nonzero++; fold = fnv(fnv(fold, c), want); }
            }
            if (diff) { snprintf(buf, sizeof buf, "BAD %llu contexts differ, first %llu: %08x != %08x", (unsigned long long)diff, (unsigned long long)first, f.S[first], lit.packed((uint32_t)first)); r = buf; }
            else if (!f.bad.empty()) r = "BAD " + f.bad;
            else if (f.replays != pairs) { snprintf(buf, sizeof buf, "BAD replays %llu, the literal replay halves in %llu (context, epoch) pairs", (unsigned long long)f.replays, (unsigned long long)pairs); r = buf; }
            else if (f.halvings != where.size()) { snprintf(buf, sizeof buf, "BAD halvings %llu != %llu", (unsigned long long)f.halvings, (unsigned long long)where.size()); r = buf; }
            else if (f.replays > 8 * n / 32767) r = "BAD more replays than 8 n / 32767";
            else {
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
