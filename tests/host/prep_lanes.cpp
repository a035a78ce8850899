// Host harness for weath3rb0i_amd/csrc/w3_prep.h (tests/test_table_prep_cpu.py): the byte histogram and StationaryModel::new the way the
// kernels compute them, compiled for the CPU.  The histogram is k_hist256's lane piece driven as a loop over the waves and their 64
// "lanes"; the stationary table is k_stat_count's lane piece summed over the lanes, then stat_walk over WaveHost (the walk's own code,
// its collectives as loops).  Every answer is compared HERE with the definition: a byte loop, and the serial loop of counter.rs:20-25 /
// stationary.rs:14-34 restated below, which also reports where the halvings fall.
//   prep_lanes <blob file> <case file>      one case per line, one answer line per case: "ok ..." or "BAD ..."
//     hist <off> <len> <a>            blob[off, off + len) copied to an address a (0 .. 15) past a 16-byte boundary, in a heap block that ends with it
//     histg <off> <len> <e>           the same flush against an inaccessible page: e = 0 starts at a page start, e = 1 ends at a page end
//     stat <off> <len> <a> [cuts..]   the stationary form of blob[off, off + len); with cuts: also as several calls cut at those byte offsets
//     statg <off> <len> <e>           the stationary form between the pages, EVERY tile through the walk's tile loader as well
//     runs <a> <len>...               runs of 0x00 and 0xFF bytes in turn (the first run is zeros), cut as `pre` cuts
//     pre <pol> <klo> <khi> <body> <a>  for every k in [klo, khi]: k bytes 0xFF (pol 0; 0x00 for pol 1) before `body` bytes 0x00 (0xFF), as one
//                                     call and as two and three calls cut at the first halving's byte, the byte behind it and the tile edges around it
//   answers: "ok h=<halvings per position> t=<the table> c=<c0:c1 per position> p<i>=<window positions of position i's halvings>"; `pre`:
//   "ok cases=<n> residues=<distinct (window position of the first halving) mod W3_STAT_TILE>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <sstream>
#include <string>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>

#define W3_HD static inline
#include "../../weath3rb0i_amd/csrc/w3_prep.h"
#include "lanes_common.h"   // Heap: a heap block that ENDS with the data, a bytes past a 16-byte boundary

struct State {
    uint32_t c0[8] = {0}, c1[8] = {0}, h[8] = {0};
    bool operator==(const State &o) const { return !memcmp(c0, o.c0, sizeof c0) && !memcmp(c1, o.c1, sizeof c1) && !memcmp(h, o.h, sizeof h); }
};

// Counter::update over the buffer (counter.rs:20-25), position 0 = the MSB; where[i] collects the byte offsets of position i's halvings
static void serial(const uint8_t *buf, size_t n, State &s, std::vector<uint64_t> *where) {
    for (size_t k = 0; k < n; k++)
        for (int i = 0; i < 8; i++) {
            const uint32_t bit = (buf[k] >> (7 - i)) & 1u;
            uint32_t &c = bit ? s.c1[i] : s.c0[i];
            if (++c == 0xFFFFu) {
                s.c0[i] = (s.c0[i] >> 1) + (s.c0[i] & 1u);
                s.c1[i] = (s.c1[i] >> 1) + (s.c1[i] & 1u);
                s.h[i]++;
                if (where) where[i].push_back(k);
            }
        }
}

// one device call: k_stat_count, then k_stat_walk for the eight positions, from the entry state s to the exit state
static void device_form(const uint8_t *p, size_t n, State &s, bool every_tile = false) {
    if (n == 0) return;
    const w3::PrepWindow win = w3::prep_window(p, n);
    const uint64_t nt = w3::stat_tiles(win);
    std::vector<uint16_t> ones8(nt * 8);
    for (uint64_t t = 0; t < nt; t++) {
        uint32_t sum[4] = {0, 0, 0, 0};
        for (uint32_t lane = 0; lane < 64; lane++) {
            uint32_t r[4];
            w3::stat_count_lane(win, t, lane, r);
            for (int j = 0; j < 4; j++) sum[j] += r[j];
        }
        for (int j = 0; j < 4; j++) { ones8[t * 8 + 2 * j] = (uint16_t)sum[j]; ones8[t * 8 + 2 * j + 1] = (uint16_t)(sum[j] >> 16); }
        if (every_tile)   // the walk's loader over this tile: the masks must agree with the counts
            for (uint32_t pos = 0; pos < 8; pos++) {
                uint32_t o = 0, v = 0;
                for (uint32_t lane = 0; lane < 64; lane++) {
                    uint64_t m, vm;
                    w3::stat_tile_lane_masks(win, t, lane, pos, m, vm);
                    if (m & ~vm) abort();
                    o += w3::prep_popc64(m); v += w3::prep_popc64(vm);
                }
                if (o != ones8[t * 8 + pos] || v != w3::stat_tile_len(win, t)) { printf("BAD tile loader: tile %llu pos %u\n", (unsigned long long)t, pos); exit(1); }
            }
    }
    w3::WaveHost wv;
    for (uint32_t pos = 0; pos < 8; pos++) w3::stat_walk(wv, p, n, ones8.data(), pos, s.c0[pos], s.c1[pos], s.h[pos]);
}

// k_hist256 + k_hist256_sum with the grid hist_workgroups picks
static void hist_form(const uint8_t *p, size_t n, uint64_t counts[256]) {
    const uint64_t nw = (uint64_t)w3::hist_workgroups(n) * 4u;
    memset(counts, 0, 256 * sizeof(uint64_t));
    for (uint64_t gw = 0; gw < nw; gw++)
        for (uint32_t lane = 0; lane < 64; lane++) w3::hist_wave_lane(p, n, lane, gw, nw, [&](uint32_t b) { counts[b]++; });
}
static std::string hist_check(const uint8_t *p, size_t n) {
    uint64_t got[256], want[256] = {0};
    hist_form(p, n, got);
    for (size_t k = 0; k < n; k++) want[p[k]]++;
    for (int v = 0; v < 256; v++)
        if (got[v] != want[v]) return "BAD hist value " + std::to_string(v) + ": " + std::to_string(got[v]) + " != " + std::to_string(want[v]);
    uint64_t fold = 1469598103934665603ull;
    for (int v = 0; v < 256; v++) fold = (fold ^ got[v]) * 1099511628211ull;
    char b[64];
    snprintf(b, sizeof b, "ok %016llx", (unsigned long long)fold);
    return b;
}

static std::string describe(const State &s, const std::vector<uint64_t> *where, uint32_t skew) {
    std::ostringstream o;
    o << "ok h=";
    for (int i = 0; i < 8; i++) o << (i ? "," : "") << s.h[i];
    o << " t=";
    for (int i = 0; i < 8; i++) o << (i ? "," : "") << w3::stat_table_entry(s.c0[i], s.c1[i]);
    o << " c=";
    for (int i = 0; i < 8; i++) o << (i ? "," : "") << s.c0[i] << ":" << s.c1[i];
    for (int i = 0; i < 8; i++) {
        o << " p" << i << "=";
        for (size_t k = 0; k < where[i].size(); k++) o << (k ? "," : "") << where[i][k] + skew;
    }
    return o.str();
}

// [p, p + n) as one call and as the calls the cut lists name (make_cuts runs behind the serial loop: it may read `where`); "" when every
// form equals the serial loop
template <class Cuts>
static std::string stat_check(const uint8_t *p, size_t n, Cuts make_cuts, State &want, std::vector<uint64_t> *where, bool every_tile = false) {
    want = State();
    serial(p, n, want, where);
    const std::vector<std::vector<size_t>> cuts = make_cuts();
    State got;
    device_form(p, n, got, every_tile);
    if (!(got == want)) return "BAD one call";
    for (const auto &cl : cuts) {
        State g;
        size_t lo = 0;
        for (size_t k = 0; k <= cl.size(); k++) {
            const size_t hi = k < cl.size() ? (cl[k] < n ? cl[k] : n) : n;
            if (hi < lo) continue;
            device_form(p + lo, hi - lo, g);
            lo = hi;
        }
        if (!(g == want)) {
            std::string s = "BAD cut at";
            for (size_t c : cl) s += " " + std::to_string(c);
            return s;
        }
    }
    return "";
}

// the cuts around byte offset h of a buffer whose window starts `skew` bytes into a chunk: at h, behind it, at the tile edges around it
static std::vector<std::vector<size_t>> cuts_around(uint64_t h, uint32_t skew) {
    const uint64_t T = W3_STAT_TILE, w = h + skew;
    const uint64_t e0 = w / T * T, e1 = e0 + T;
    std::vector<std::vector<size_t>> c = {{(size_t)h}, {(size_t)h + 1}, {(size_t)h, (size_t)h + 1}, {(size_t)h, (size_t)(e1 - skew)}};
    if (e0 >= skew) c.push_back({(size_t)(e0 - skew), (size_t)h + 1});
    return c;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: prep_lanes <blob> <cases>\n"); return 2; }
    std::vector<uint8_t> blob;
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
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    const size_t gpages = (4096 + page - 1) / page + 1;   // room for the guarded cases (up to 4 KiB)
    uint8_t *m = (uint8_t *)mmap(nullptr, (gpages + 2) * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) { perror("mmap"); return 2; }
    if (mprotect(m, page, PROT_NONE) || mprotect(m + (gpages + 1) * page, page, PROT_NONE)) { perror("mprotect"); return 2; }
    uint8_t *lo = m + page, *hi = m + (gpages + 1) * page;
    FILE *cf = fopen(argv[2], "r");
    if (!cf) { perror(argv[2]); return 2; }
    static char line[1 << 16];
    while (fgets(line, sizeof line, cf)) {
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        unsigned long long a = 0, b = 0, c = 0;
        if (kind == "hist" || kind == "histg") {
            in >> a >> b >> c;
            if (!in || a + b > blob.size()) return 2;
            if (kind == "hist") {
                if (c > 15) return 2;
                Heap h((size_t)b, (unsigned)c);
                if (b) memcpy(h.p, blob.data() + a, (size_t)b);
                puts(hist_check(h.p, (size_t)b).c_str());
            } else {
                if (b > 4096) return 2;
                uint8_t *p = c ? hi - b : lo;
                if (b) memcpy(p, blob.data() + a, (size_t)b);
                puts(hist_check(p, (size_t)b).c_str());
            }
        } else if (kind == "stat" || kind == "statg") {
            in >> a >> b >> c;
            if (!in || a + b > blob.size()) return 2;
            State want;
            std::vector<uint64_t> where[8];
            std::string r;
            if (kind == "stat") {
                if (c > 15) return 2;
                std::vector<std::vector<size_t>> cuts;
                std::vector<size_t> cl;
                unsigned long long x;
                while (in >> x) cl.push_back((size_t)x);
                if (!cl.empty()) cuts.push_back(cl);
                Heap h((size_t)b, (unsigned)c);
                if (b) memcpy(h.p, blob.data() + a, (size_t)b);
                r = stat_check(h.p, (size_t)b, [&] { return cuts; }, want, where);
                if (r.empty()) r = describe(want, where, (uint32_t)c);
            } else {
                if (b > 4096) return 2;
                uint8_t *p = c ? hi - b : lo;
                if (b) memcpy(p, blob.data() + a, (size_t)b);
                r = stat_check(p, (size_t)b, [] { return std::vector<std::vector<size_t>>(); }, want, where, true);
                if (r.empty()) r = describe(want, where, (uint32_t)((uintptr_t)p & 15u));
            }
            puts(r.c_str());
        } else if (kind == "runs") {
            in >> a;
            if (!in || a > 15) return 2;
            std::vector<size_t> runs;
            size_t n = 0;
            unsigned long long x;
            while (in >> x) { runs.push_back((size_t)x); n += (size_t)x; }
            Heap h(n, (unsigned)a);
            size_t o = 0;
            for (size_t k = 0; k < runs.size(); k++) { memset(h.p + o, k & 1 ? 0xFF : 0x00, runs[k]); o += runs[k]; }
            State want;
            std::vector<uint64_t> where[8];
            std::string r = stat_check(h.p, n, [&] {
                std::vector<std::vector<size_t>> cuts;
                for (uint64_t w : where[0])
                    for (auto &cl : cuts_around(w, (uint32_t)a)) cuts.push_back(cl);
                return cuts;
            }, want, where);
            if (r.empty()) r = describe(want, where, (uint32_t)a);
            puts(r.c_str());
        } else if (kind == "pre") {
            unsigned long long pol = 0, klo = 0, khi = 0, body = 0, al = 0;
            in >> pol >> klo >> khi >> body >> al;
            if (!in || al > 15 || khi < klo) return 2;
            std::set<uint64_t> residues;
            unsigned long long ncases = 0;
            std::string r;
            for (unsigned long long k = klo; k <= khi && r.empty(); k++) {
                const size_t n = (size_t)(k + body);
                Heap h(n, (unsigned)al);
                memset(h.p, pol ? 0x00 : 0xFF, (size_t)k);
                memset(h.p + k, pol ? 0xFF : 0x00, (size_t)body);
                State want;
                std::vector<uint64_t> where[8];
                r = stat_check(h.p, n, [&] {
                    std::vector<std::vector<size_t>> cuts;
                    if (!where[0].empty()) { cuts = cuts_around(where[0][0], (uint32_t)al); residues.insert((where[0][0] + al) % W3_STAT_TILE); }
                    return cuts;
                }, want, where);
                if (!r.empty()) r += " (k = " + std::to_string(k) + ")";
                ncases++;
            }
            if (r.empty()) r = "ok cases=" + std::to_string(ncases) + " residues=" + std::to_string(residues.size());
            puts(r.c_str());
        } else {
            fprintf(stderr, "bad case: %s", line);
            return 2;
        }
        fflush(stdout);
    }
    fclose(cf);
    return 0;
}
