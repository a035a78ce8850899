// match_round.cpp — the match-model leaf's index arithmetic (weath3rb0i_amd/csrc/w3_match_plan.h) on the host: blocks walked in
// k_match_keys' ROUND order — 64 simulated lanes per round, every lane reading the tables' state before the round, equal hashes resolved
// by the nearest-lower-lane rule, only the highest lane of a group storing, entries tagged with the wavefront's block sequence — and in the
// lane kernels' serial order (match_advance, knowing only the bytes before the boundary), both against the serial definition written out
// here byte by byte.  Every byte index a header load touches is asserted inside [0, known) of its block, and every block lies in a heap
// buffer of exactly its size.  Stand-alone: tests/test_match_round.py builds it with g++, once more under -fsanitize=undefined,address,
// and with mutant headers that must fail.  One wavefront's life over mixed blocks wraps the tags; a second part walks STEERED inputs (what
// tests/match_ref.py: tag_blocks builds for the GPU test) — the blocks at sequence 0, 255, 510 one phrase, whose table entries no other block
// touches, so that only the re-zeroing at the wrap and the tag check keep them from passing for candidates, some of them past the boundary
// that looks them up or past a short last block's end — and one block of 70,000 bytes whose entries hold positions above bit 16.
// usage: match_round [blocks per shape]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 10) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint64_t n_loads = 0;
static void check_idx(uint32_t first, uint32_t count, uint32_t known) {
    n_loads++;
    CHECK((uint64_t)first + count <= known, "load of bytes [%u, %u) in a block of %u known bytes", first, first + count, known);
}
#define W3_MATCH_CHECK(first, count, known) check_idx(first, count, known)
#include "../../weath3rb0i_amd/csrc/w3_match_plan.h"

// ---- the serial definition -------------------------------------------------------------------------------------------------------------
struct Pred { uint32_t v, e, lq; };

static uint32_t def_hash(const uint8_t *x, uint32_t i, uint32_t k, uint32_t L) {
    uint64_t v = 0;
    for (uint32_t s = 0; s < k; s++) v = (v << 8) | x[i - k + s];
    return (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> (64 - L));
}
static uint32_t def_len(const uint8_t *x, uint32_t i, uint32_t c) {
    if (c == 0) return 0;
    const uint32_t limit = c < 32u ? c : 32u;
    uint32_t r = 0;
    while (r < limit && x[i - 1 - r] == x[c - 1 - r]) r++;
    return r;
}
static std::vector<Pred> definition(const uint8_t *x, uint32_t n, uint32_t m, uint32_t L) {
    std::vector<uint32_t> T[2] = {std::vector<uint32_t>((size_t)1 << L, 0u), std::vector<uint32_t>((size_t)1 << L, 0u)};
    std::vector<Pred> out(n);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t c[2] = {0, 0}, v[2] = {0, 0};
        for (uint32_t t = 0; t < 2; t++) {
            const uint32_t k = m << t;
            if (i < k) continue;
            const uint32_t h = def_hash(x, i, k, L);
            c[t] = T[t][h];
            T[t][h] = i;
            v[t] = def_len(x, i, c[t]);
        }
        const uint32_t t = v[1] > v[0] ? 1u : 0u;
        out[i].v = v[t];
        out[i].e = v[t] ? x[c[t]] : 0u;
        out[i].lq = v[t] == 0 ? 0u : v[t] < 16 ? v[t] : 16 + ((v[t] - 16) >> 2);
    }
    return out;
}
static uint32_t def_key(const Pred &p, uint32_t byte, uint32_t j) {
    if (p.v == 0 || (byte >> (8 - j)) != (p.e >> (8 - j))) return 0;
    return (p.lq << 1) | ((p.e >> (7 - j)) & 1);
}

// ---- the kernel's walk: one wavefront, its blocks one after the other over the same two tables ------------------------------------------
struct Wave {
    uint32_t m, L, seq = 0;
    uint64_t stale_rejected = 0, stale_past_boundary = 0, stale_past_end = 0, zeroings = 0, far_positions = 0;
    std::vector<uint32_t> tbl;
    Wave(uint32_t m_, uint32_t L_) : m(m_), L(L_), tbl((size_t)2 << L_, 0xDEADBEEFu) {}   // (the kernel zeroes them at tag 1: garbage until then)

    void block(const uint8_t *blk, uint32_t len, const std::vector<Pred> &want, const char *what) {
        using namespace w3;
        const uint32_t tag = seq % W3_MATCH_TAGS + 1u;
        seq++;
        if (tag == 1u) { std::fill(tbl.begin(), tbl.end(), 0u); zeroings++; }
        for (uint32_t base = 0; base < len; base += 64u) {
            uint32_t c[2][64], v[2][64];
            for (uint32_t t = 0; t < 2u; t++) {
                const uint32_t k = m << t;
                bool act[64]; uint32_t h[64], old[64];
                for (uint32_t lane = 0; lane < 64u; lane++) {   // every lane's hash and load: the state before the round
                    const uint32_t i = base + lane;
                    act[lane] = i < len && i >= k;
                    h[lane] = act[lane] ? match_hash(match_window(blk, len, i), k, L) : 0u;
                    old[lane] = act[lane] ? tbl[((size_t)t << L) + h[lane]] : 0u;
                    if (act[lane]) CHECK(h[lane] == def_hash(blk, i, k, L), "%s: hash of boundary %u, k %u", what, i, k);
                }
                for (uint32_t lane = 0; lane < 64u; lane++) {
                    const uint32_t i = base + lane;
                    uint64_t M = 0;   // (the ballots' result)
                    for (uint32_t o = 0; o < 64u; o++)
                        if (act[o] && h[o] == h[lane]) M |= 1ull << o;
                    const int nl = match_nearest_lower(M, lane);
                    c[t][lane] = !act[lane] ? 0u : nl >= 0 ? base + (uint32_t)nl : match_entry_pos(tag, old[lane]);
                    v[t][lane] = act[lane] ? match_length(blk, len, i, c[t][lane]) : 0u;
                    if (act[lane] && nl < 0 && old[lane] != 0u && (old[lane] >> 24) != tag) {   // an earlier block's entry: what the tag is for
                        stale_rejected++;
                        stale_past_boundary += (old[lane] & 0xFFFFFFu) >= i;
                        stale_past_end += (old[lane] & 0xFFFFFFu) > len;
                    }
                    far_positions += c[t][lane] >= 65536u;
                }
                for (uint32_t lane = 0; lane < 64u; lane++) {   // the stores, after every load of the round
                    uint64_t M = 0;
                    for (uint32_t o = 0; o < 64u; o++)
                        if (act[o] && h[o] == h[lane]) M |= 1ull << o;
                    if (act[lane] && match_is_writer(M, lane)) tbl[((size_t)t << L) + h[lane]] = match_entry(tag, base + lane);
                }
            }
            for (uint32_t lane = 0; lane < 64u && base + lane < len; lane++) {
                const uint32_t i = base + lane;
                const uint32_t t = match_takes_long(v[0][lane], v[1][lane]) ? 1u : 0u;
                const uint32_t vv = v[t][lane], lq = vv ? match_lq(vv) : 0u, e = vv ? blk[c[t][lane]] : 0u;
                CHECK(vv == want[i].v && lq == want[i].lq && e == want[i].e, "%s: boundary %u of %u (m %u, L %u): v %u lq %u e %u, definition %u %u %u", what, i, len,
                      m, L, vv, lq, e, want[i].v, want[i].lq, want[i].e);
                for (uint32_t j = 0; j < 8u; j++)
                    CHECK(match_key(lq, e, (uint32_t)blk[i] >> (8u - j), j) == def_key(want[i], blk[i], j), "%s: key %u of byte %u", what, j, i);
            }
        }
    }
};

// the lane kernels' order: boundary i from the bytes [0, i) alone (a decoder has no more)
static void serial(const uint8_t *blk, uint32_t len, uint32_t m, uint32_t L, const std::vector<Pred> &want, const char *what) {
    std::vector<uint32_t> T((size_t)2 << L, 0u);
    w3::MatchState s;
    for (uint32_t i = 1; i < len; i++) {
        w3::match_advance(s, T.data(), m, L, blk, i, i);
        CHECK(s.lq == want[i].lq && s.e == want[i].e, "%s: serial boundary %u: lq %u e %u, definition %u %u", what, i, s.lq, s.e, want[i].lq, want[i].e);
    }
}

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 16); }

// shape 0: one byte value; 1: period p; 2..4: alphabets of 2, 16, 256 symbols; 5: words; 6: a long repeat of an earlier stretch
static void fill(uint8_t *x, uint32_t n, uint32_t shape) {
    static const char *words[] = {"the ", "quick ", "brown ", "fox ", "jumps ", "over ", "a ", "lazy ", "dog. "};
    const uint32_t p = 1 + rnd() % 70, val = rnd() & 255u;
    uint32_t i = 0;
    switch (shape) {
    case 0: memset(x, (int)val, n); break;
    case 1: for (; i < n; i++) x[i] = (uint8_t)(i % p * 37u + val); break;
    case 2: case 3: case 4: for (; i < n; i++) x[i] = (uint8_t)(rnd() % (shape == 2 ? 2u : shape == 3 ? 16u : 256u)); break;
    case 5: while (i < n) { const char *w = words[rnd() % 9]; for (; *w && i < n; w++) x[i++] = (uint8_t)*w; } break;
    default:
        for (; i < n; i++) x[i] = (uint8_t)rnd();
        if (n > 100) { const uint32_t len = n / 3, src = rnd() % (n / 3), dst = n - len; memmove(x + dst, x + src, len); }
    }
}

// ---- the steered inputs ------------------------------------------------------------------------------------------------------------------
// bs bytes without structure, but for one stretch of 2m + 1 bytes met twice (in the second round where there is one): an equal block's
// entry for the contexts behind it lies past the first boundary that looks it up
static std::vector<uint8_t> phrase(uint32_t bs, uint32_t m, uint32_t seed) {
    std::vector<uint8_t> p(bs);
    uint32_t s = seed * 2654435761u + 1u;
    for (uint32_t i = 0; i < bs; i++) { s = s * 1103515245u + 12345u; p[i] = (uint8_t)(s >> 16); }
    const uint32_t r = bs <= 64u ? bs / 2u : 64u, k = 2u * m + 1u < bs - r ? 2u * m + 1u : bs - r;
    memcpy(p.data() + r, p.data(), k);
    return p;
}
static bool share_an_entry(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, uint32_t m, uint32_t L) {
    for (uint32_t t = 0; t < 2; t++)
        for (uint32_t i = m << t; i < a.size(); i++)
            for (uint32_t j = m << t; j < b.size(); j++)
                if (def_hash(a.data(), i, m << t, L) == def_hash(b.data(), j, m << t, L)) return true;
    return false;
}
static void walk_one(Wave &wave, const uint8_t *src, uint32_t n, const char *what) {
    uint8_t *x = (uint8_t *)malloc(n);   // exactly the block
    memcpy(x, src, n);
    const std::vector<Pred> want = definition(x, n, wave.m, wave.L);
    wave.block(x, n, want, what);
    free(x);
}
static uint64_t steered() {
    static const uint32_t cases[4][5] = {{520, 24, 12, 2, 12}, {520, 72, 0, 2, 12}, {300, 40, 0, 4, 16}, {520, 24, 0, 2, 8}};   // blocks, size, tail, m, L
    uint64_t blocks = 0;
    for (const auto &cs : cases) {
        const uint32_t nb = cs[0], bs = cs[1], tail = cs[2], m = cs[3], L = cs[4];
        const std::vector<uint8_t> A = phrase(bs, m, 1);
        std::vector<uint8_t> other[2];
        for (uint32_t seed = 2, k = 0; k < 2; seed++) {
            std::vector<uint8_t> p = phrase(bs, m, seed);
            if (!share_an_entry(A, p, m, L)) other[k++] = p;
        }
        Wave wave(m, L);
        char what[64];
        for (uint32_t b = 0; b < nb + (tail ? 1u : 0u); b++, blocks++) {
            const std::vector<uint8_t> &p = b % W3_MATCH_TAGS == 0 ? A : other[b & 1u];
            snprintf(what, sizeof what, "steered %ux%u block %u", nb, bs, b);
            walk_one(wave, p.data(), b < nb ? bs : tail, what);
        }
        CHECK(wave.zeroings == (nb + (tail ? 1u : 0u) - 1u) / W3_MATCH_TAGS + 1u && wave.zeroings >= 2, "steered %ux%u: %llu zeroings", nb, bs, (unsigned long long)wave.zeroings);
        CHECK(wave.stale_rejected > nb && wave.stale_past_boundary > 0, "steered %ux%u: %llu stale entries rejected, %llu at or past the boundary", nb, bs,
              (unsigned long long)wave.stale_rejected, (unsigned long long)wave.stale_past_boundary);
        CHECK(!tail || wave.stale_past_end > 0, "steered %ux%u: no stale entry past the short last block's end", nb, bs);
    }
    // one long block: a 40-byte phrase near the start, past offset 65,536 and once more behind that
    {
        const uint32_t n = 70000;
        std::vector<uint8_t> x(n);
        for (uint32_t i = 0; i < n; i++) x[i] = (uint8_t)rnd();
        for (uint32_t o : {66000u, 68500u}) memcpy(x.data() + o, x.data() + 100, 40);
        Wave wave(4, 20);
        walk_one(wave, x.data(), n, "long block");
        CHECK(wave.far_positions > 0, "long block: no candidate at position 65,536 or above");
        const std::vector<Pred> want = definition(x.data(), n, 4, 20);
        serial(x.data(), n, 4, 20, want, "long block");
        blocks++;
    }
    return blocks;
}

int main(int argc, char **argv) {
    const uint32_t reps = argc > 1 ? (uint32_t)atoi(argv[1]) : 3u;
    static const uint32_t sizes[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1000, 4096};
    static const uint32_t cfg[3][2] = {{2, 8}, {3, 12}, {4, 16}};
    uint64_t blocks = 0;
    for (uint32_t ci = 0; ci < 3; ci++) {
        Wave wave(cfg[ci][0], cfg[ci][1]);   // one wavefront's life: every block below in turn, its tags wrapping past 255
        for (uint32_t rep = 0; rep < reps; rep++)
            for (uint32_t shape = 0; shape < 7; shape++)
                for (uint32_t n : sizes) {
                    uint8_t *x = (uint8_t *)malloc(n);   // exactly the block: a load outside it is the sanitizer's
                    fill(x, n, shape);
                    char what[64];
                    snprintf(what, sizeof what, "shape %u size %u rep %u", shape, n, rep);
                    const std::vector<Pred> want = definition(x, n, cfg[ci][0], cfg[ci][1]);
                    wave.block(x, n, want, what);
                    serial(x, n, cfg[ci][0], cfg[ci][1], want, what);
                    free(x);
                    blocks++;
                }
        CHECK(reps < 2 || wave.seq > W3_MATCH_TAGS, "the tags did not wrap: %u blocks", wave.seq);
    }
    blocks += steered();
    // the length bucket and the rules, spelled out
    for (uint32_t v = 1; v <= 32; v++) CHECK(w3::match_lq(v) == (v < 16 ? v : 16 + (v - 16) / 4) && w3::match_lq(v) <= 20, "lq(%u)", v);
    CHECK(w3::match_nearest_lower(0x8000000000000001ull, 63) == 0 && w3::match_nearest_lower(1ull, 0) == -1 && w3::match_nearest_lower(0xFFull, 5) == 4, "nearest lower lane");
    CHECK(w3::match_is_writer(0x8000000000000001ull, 63) && !w3::match_is_writer(0x8000000000000001ull, 0) && w3::match_is_writer(1ull, 0), "writer");
    CHECK(w3::match_takes_long(3, 4) && !w3::match_takes_long(4, 4) && !w3::match_takes_long(5, 4), "long wins only if strictly longer");
    CHECK(w3::match_entry_pos(7, w3::match_entry(7, 0xABCDEF)) == 0xABCDEF && w3::match_entry_pos(8, w3::match_entry(7, 5)) == 0 && w3::match_entry_pos(1, 0) == 0, "tags");
    if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
    printf("match round ok: %llu blocks, %llu checked loads\n", (unsigned long long)blocks, (unsigned long long)n_loads);
    return 0;
}
