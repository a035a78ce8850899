// What the host harnesses of this directory share (prep_lanes.cpp, export_lanes.cpp, export_entropy_lanes.cpp): the Counter of the literal
// yardsticks, the buffers that catch a read outside the input, the case files' inputs, and — for the two export harnesses, which include
// weath3rb0i_amd/csrc/w3_export.h first and define LANES_EXPORT_FORM — the device form of a piece: count, apply and replay per epoch
// over a step source.  Nothing here is a yardstick: the literal restatements stay in the harnesses.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>

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
struct Halving { uint64_t byte; uint32_t ctx; };   // where a literal run halved

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
// f(p) with src[0 .. n) copied to a buffer of its own: a = 0 .. 15 a Heap at that skew, 16 / 17 Guarded at a page start / a page end
template <class F>
static inline void in_buffer(const uint8_t *src, size_t n, unsigned a, F f) {
    if (a <= 15) {
        Heap h(n, a);
        if (n) memcpy(h.p, src, n);
        f((const uint8_t *)h.p);
    } else {
        Guarded g(n, a == 17);
        if (n) memcpy(g.p, src, n);
        f((const uint8_t *)g.p);
    }
}

static inline bool load_blob(const char *path, std::vector<uint8_t> &blob) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return false; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    blob.resize((size_t)n);
    const bool ok = !n || fread(blob.data(), 1, (size_t)n, f) == (size_t)n;
    if (!ok) perror("read");
    fclose(f);
    return ok;
}

// <input>: blob:<off>:<len> | ffz:<p>:<len> (p bytes 0xFF, then len zero bytes) | zrun:<a>:<z>:<f>:<b> (blob[0:a], z zero bytes, f bytes
// 0xFF, blob[a:a+b])
static inline bool make_input(const std::vector<uint8_t> &blob, const std::string &spec, std::vector<uint8_t> &out) {
    unsigned long long a = 0, b = 0, c = 0, d = 0;
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
    if (sscanf(spec.c_str(), "zrun:%llu:%llu:%llu:%llu", &a, &b, &c, &d) == 4) {
        if (a + d > blob.size()) return false;
        out.assign(blob.begin(), blob.begin() + (long)a);
        out.insert(out.end(), (size_t)b, 0);
        out.insert(out.end(), (size_t)c, 0xFF);
        out.insert(out.end(), blob.begin() + (long)a, blob.begin() + (long)(a + d));
        return true;
    }
    return false;
}

static const uint64_t FNV0 = 1469598103934665603ull;
static inline uint64_t fnv(uint64_t h, uint64_t v) { return (h ^ v) * 1099511628211ull; }

// the pieces [lo, hi) the cut list makes of n bytes
static inline std::vector<std::pair<uint64_t, uint64_t>> pieces_of(uint64_t n, const std::vector<uint64_t> &cuts) {
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

// (context, epoch) pairs in which a literal run halves, for pieces cut as above with epochs of E bytes from every piece's start
static inline uint64_t literal_pairs(const std::vector<Halving> &where, const std::vector<std::pair<uint64_t, uint64_t>> &pieces, uint64_t E) {
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

#ifdef LANES_EXPORT_FORM   // (the export harnesses define it, after including w3_export.h)
// The device form of the export: D, S and the counts a call reports
struct Form {
    w3::ExpModel m;
    std::vector<uint64_t> D;
    std::vector<uint32_t> S;
    uint64_t replays = 0, halvings = 0, epochs = 0;
    std::string bad;
    Form(uint32_t bits, uint32_t align) : m{bits, align}, D((size_t)1 << bits), S((size_t)1 << bits) {}
    // One piece, as a device call runs it: per epoch k_exp_count (here: 7 waves striding over the rows), k_ctx_apply, k_exp_replay over
    // the step source source(e0, len) gives for the epoch — which is where a key stage runs.
    template <class Source>
    void piece(const w3::ExpPiece &pc, uint64_t E, Source source) {
        std::vector<uint32_t> touched, list;
        for (uint64_t e0 = 0; e0 < pc.n; e0 += E) {
            const uint64_t len = std::min<uint64_t>(E, pc.n - e0);
            const auto src = source(e0, len);
            const uint64_t nw = 7;
            touched.clear();
            for (uint64_t gw = 0; gw < nw; gw++)
                for (uint32_t lane = 0; lane < 64; lane++)
                    w3::exp_count_wave_lane(src, lane, gw, nw, [&](uint32_t ctx, uint32_t bit) {
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
                const uint32_t h = w3::exp_replay(wv, src, c, S[c]);
                if (!h) bad = "a listed context without a halving";
                halvings += h;
            }
            replays += list.size();
            epochs++;
        }
    }
    // what is left to say once the pieces are through: S against the literal table want(c), D, replays against the literal's (context,
    // epoch) pairs, halvings against the literal's; "" if all of it holds
    template <class Want>
    std::string verdict(Want want, uint64_t pairs, uint64_t lit_halvings, uint64_t n) {
        uint64_t diff = 0, first = 0;
        for (uint32_t c = 0; c < S.size(); c++) {
            if (S[c] != want(c) && !diff++) first = c;
            if (D[c]) bad = "D is not left zeroed";
        }
        char buf[256] = "";
        if (!bad.empty()) return "BAD " + bad;
        if (diff) snprintf(buf, sizeof buf, "BAD %llu contexts differ, first %llu: %08x != %08x", (unsigned long long)diff, (unsigned long long)first, S[first], want((uint32_t)first));
        else if (replays != pairs) snprintf(buf, sizeof buf, "BAD replays %llu, the literal run halves in %llu (context, epoch) pairs", (unsigned long long)replays, (unsigned long long)pairs);
        else if (halvings != lit_halvings) snprintf(buf, sizeof buf, "BAD halvings %llu != %llu", (unsigned long long)halvings, (unsigned long long)lit_halvings);
        else if (replays > 8 * n / 32767) return "BAD more replays than 8 n / 32767";
        return buf;
    }
};
#endif
