// Host harness for weath3rb0i_amd/csrc/w3_aoh_plan.h (tests/test_aoh_plan.py): the two bit-string helpers and the batch plan of the
// two-phase form of AC over Huffman, compiled for the CPU.
//   Strings: for seeded random canonical code tables (longest code 1 .. 16 bits, absent symbols included) and seeded random blocks, the
//   block is packed with aoh_put_code — the codes in a SHUFFLED order, as k_aoh_pack's lanes may arrive — into a region of exactly
//   aoh_str_bytes(L) bytes; then every step's (context, bit) is taken as k_aoh_predict takes it (aoh_window / aoh_step_ctx / aoh_step_bit)
//   and the bit as k_aoh_coder takes it (big-endian words), and compared with a literal restatement of the driver's loop
//   (bin/ac-over-huffman/main.rs:79-84): walk each code MSB first, ctx = hist & mask, hist = hist << 1 | bit.
//   Plan: offsets aligned, non-overlapping, in block order; every block in exactly one batch; batches within the budget and the block
//   cap, and closed only when the next block would not fit; 64-bit offsets.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../weath3rb0i_amd/csrc/w3_aoh_plan.h"

static unsigned long g_checks = 0;
#define CHECK(cond, ...)                                                                \
    do {                                                                                \
        g_checks++;                                                                     \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond);        \
            std::fprintf(stderr, __VA_ARGS__);                                          \
            std::fprintf(stderr, "\n");                                                 \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

struct Table { uint16_t code[256]; uint8_t len[256]; };

// canonical codes from lengths: the first code of every length from the length counts, symbols of one length in ascending order
static void canonical(Table &t) {
    uint32_t cnt[18] = {0}, next[18] = {0};
    for (int s = 0; s < 256; s++) if (t.len[s]) cnt[t.len[s]]++;
    for (int l = 0; l < 16; l++) next[l + 1] = (next[l] + cnt[l]) << 1;
    for (int s = 0; s < 256; s++) t.code[s] = t.len[s] ? (uint16_t)next[t.len[s]]++ : 0;
}

// a random complete prefix code: split random leaves no deeper than max_len until there are `nsym` of them, on random symbols
static Table random_table(std::mt19937_64 &rng, unsigned max_len, unsigned nsym) {
    std::vector<unsigned> depth{1, 1};
    if (nsym < 2) depth.assign(1, 1);           // one symbol: a 1-bit code (the container writer's replacement table)
    while (depth.size() < nsym) {
        std::vector<size_t> can;
        for (size_t i = 0; i < depth.size(); i++) if (depth[i] < max_len) can.push_back(i);
        if (can.empty()) break;
        const size_t i = can[rng() % can.size()];
        depth[i]++;
        depth.push_back(depth[i]);
    }
    std::vector<int> syms(256);
    for (int s = 0; s < 256; s++) syms[s] = s;
    std::shuffle(syms.begin(), syms.end(), rng);
    Table t;
    memset(&t, 0, sizeof t);
    for (size_t i = 0; i < depth.size(); i++) t.len[syms[i]] = (uint8_t)depth[i];
    canonical(t);
    for (int s = 0; s < 256; s++) CHECK(t.len[s] <= 16 && !(t.code[s] >> t.len[s]), "table: symbol %d", s);
    return t;
}

static const uint32_t CTX_BITS[] = {1, 8, 19, 24, 31};

static void run_block(const Table &t, const std::vector<uint8_t> &blk, std::mt19937_64 &rng, const char *what) {
    // the driver's loop, literally: (bit, history before it) of every step
    std::vector<uint8_t> want_bit;
    std::vector<uint32_t> want_hist;
    uint32_t hist = 0;
    for (uint8_t byte : blk)
        for (int i = (int)t.len[byte] - 1; i >= 0; i--) {
            const uint32_t bit = (t.code[byte] >> i) & 1u;
            want_bit.push_back((uint8_t)bit);
            want_hist.push_back(hist);
            hist = (hist << 1) | bit;
        }
    const uint64_t L = want_bit.size();
    // pack: bit offsets by prefix sum, the codes in any order, OR into big-endian words of a region of exactly the planned size
    std::vector<uint64_t> q(blk.size());
    uint64_t sum = 0;
    for (size_t i = 0; i < blk.size(); i++) { q[i] = sum; sum += t.len[blk[i]]; }
    CHECK(sum == L, "%s: L", what);
    const uint64_t region_bytes = w3::aoh_str_bytes((uint32_t)L);
    CHECK(region_bytes % w3::AOH_STR_ALIGN == 0 && region_bytes >= w3::AOH_STR_PAD + (L + 7) / 8 + 4, "%s: region of %llu bytes for %llu bits", what,
          (unsigned long long)region_bytes, (unsigned long long)L);
    std::vector<uint8_t> region(region_bytes, 0);
    uint8_t *bits = region.data() + w3::AOH_STR_PAD;
    const uint64_t words = (region_bytes - w3::AOH_STR_PAD) / 4;
    std::vector<size_t> order(blk.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    for (size_t i : order)
        w3::aoh_put_code(t.code[blk[i]], t.len[blk[i]], q[i], [&](uint64_t w, uint32_t v) {
            CHECK(w < words, "%s: word %llu outside the region (%llu words)", what, (unsigned long long)w, (unsigned long long)words);
            for (int k = 0; k < 4; k++) bits[4 * w + k] |= (uint8_t)(v >> (24 - 8 * k));
        });
    for (uint32_t k = 0; k < w3::AOH_STR_PAD; k++) CHECK(region[k] == 0, "%s: padding byte %u written", what, k);
    for (uint64_t k = (L + 7) / 8; k < region_bytes - w3::AOH_STR_PAD; k++) CHECK(bits[k] == 0, "%s: byte %llu behind the string not zero", what, (unsigned long long)k);
    if (L & 7) CHECK((bits[L >> 3] & (0xFFu >> (L & 7))) == 0, "%s: bits behind the string's end set", what);
    // every step as the predict kernel takes it, for every context width; the bit also as the coder takes it
    for (uint32_t cb : CTX_BITS) {
        const uint32_t mask = (uint32_t)((1ull << cb) - 1ull);
        for (uint64_t s = 0; s < L; s++) {
            const uint64_t W = w3::aoh_window(bits, s);
            const uint32_t bit = w3::aoh_step_bit(W, s), ctx = w3::aoh_step_ctx(W, s, mask);
            CHECK(bit == want_bit[s], "%s: step %llu bit", what, (unsigned long long)s);
            CHECK(ctx == (want_hist[s] & mask), "%s: step %llu ctx_bits %u: context %08x want %08x", what, (unsigned long long)s, cb, ctx, want_hist[s] & mask);
        }
    }
    for (uint64_t s = 0; s < L; s++) {
        const uint32_t g = (uint32_t)(s >> 3), j = (uint32_t)s & 7u;
        uint32_t raw;
        memcpy(&raw, bits + 4 * (g >> 2), 4);
        const uint32_t w = __builtin_bswap32(raw), byte = (w >> (24u - 8u * (g & 3u))) & 0xFFu;
        CHECK(((byte >> (7u - j)) & 1u) == want_bit[s], "%s: step %llu bit by words", what, (unsigned long long)s);
    }
}

static void string_cases(uint64_t seed, int rounds) {
    std::mt19937_64 rng(seed);
    for (int r = 0; r < rounds; r++) {
        const unsigned max_len = 1 + r % 16, nsym = 1 + (unsigned)(rng() % 256);
        const Table t = random_table(rng, max_len, nsym);
        std::vector<int> present;
        for (int s = 0; s < 256; s++) if (t.len[s]) present.push_back(s);
        const size_t n = rng() % 700;
        std::vector<uint8_t> blk(n);
        const bool with_absent = r % 3 == 0;     // bytes whose len is 0 contribute nothing (the counting sink mirrors the reference)
        for (auto &c : blk) c = with_absent && rng() % 8 == 0 ? (uint8_t)(rng() % 256) : (uint8_t)present[rng() % present.size()];
        run_block(t, blk, rng, "random");
    }
    // L_b = 0, 1, 63, 64, 65 and a long block of one repeated 1-bit code (either bit value); then the same lengths from 16-bit codes
    Table two;
    memset(&two, 0, sizeof two);
    two.len['a'] = 1; two.len['b'] = 1;
    canonical(two);
    CHECK(two.code['a'] == 0 && two.code['b'] == 1, "two-symbol table");
    for (size_t n : {0u, 1u, 63u, 64u, 65u, 5000u})
        for (uint8_t c : {(uint8_t)'a', (uint8_t)'b'}) run_block(two, std::vector<uint8_t>(n, c), rng, "one repeated 1-bit code");
    run_block(two, std::vector<uint8_t>(100, (uint8_t)'z'), rng, "absent symbols only: L = 0");
    {
        std::vector<uint8_t> mixed(65);
        for (size_t i = 0; i < mixed.size(); i++) mixed[i] = (rng() & 1) ? 'a' : 'b';
        for (size_t n : {1u, 63u, 64u, 65u}) run_block(two, std::vector<uint8_t>(mixed.begin(), mixed.begin() + (long)n), rng, "1-bit codes");
    }
    const Table deep = random_table(rng, 16, 256);
    std::vector<int> longest;
    for (int s = 0; s < 256; s++) if (deep.len[s] == 16) longest.push_back(s);
    CHECK(!longest.empty(), "a 16-bit code");
    for (size_t n : {1u, 4u, 5u, 300u}) {
        std::vector<uint8_t> blk(n);
        for (auto &c : blk) c = (uint8_t)longest[rng() % longest.size()];
        run_block(deep, blk, rng, "16-bit codes");
    }
}

static void check_plan(const std::vector<uint32_t> &L, uint64_t budget, uint32_t cap, const char *what) {
    w3::AohPlan p;
    const size_t nb = L.size();
    uint64_t largest = 0;
    for (uint32_t l : L) largest = std::max(largest, w3::AohPlan::bytes(w3::aoh_str_bytes(l), w3::aoh_p_steps(l)));
    const bool ok = w3::aoh_plan(L.data(), nb, budget, cap, p);
    CHECK(ok == (largest <= budget), "%s: plan %d, largest block %llu, budget %llu", what, (int)ok, (unsigned long long)largest, (unsigned long long)budget);
    if (!ok) return;
    CHECK(p.str_off.size() == nb && p.p_off.size() == nb, "%s: sizes", what);
    std::vector<int> seen(nb, 0);
    uint32_t next = 0;
    uint64_t max_s = 0, max_p = 0;
    for (size_t k = 0; k < p.batches.size(); k++) {
        const w3::AohBatch &bt = p.batches[k];
        CHECK(bt.count > 0 && bt.first == next, "%s: batch %zu starts at %u, want %u", what, k, bt.first, next);
        CHECK(!cap || bt.count <= cap, "%s: batch %zu holds %u blocks, cap %u", what, k, bt.count, cap);
        uint64_t s = 0, ps = 0;
        for (uint32_t b = bt.first; b < bt.first + bt.count; b++) {
            CHECK(b < nb, "%s: block %u", what, b);
            seen[b]++;
            CHECK(p.str_off[b] == s && p.p_off[b] == ps, "%s: block %u offsets (%llu, %llu) want (%llu, %llu)", what, b, (unsigned long long)p.str_off[b],
                  (unsigned long long)p.p_off[b], (unsigned long long)s, (unsigned long long)ps);
            CHECK(p.str_off[b] % w3::AOH_STR_ALIGN == 0 && p.p_off[b] % w3::AOH_P_ALIGN == 0, "%s: block %u alignment", what, b);
            // the region holds the padding, the string and the word the coder reads ahead; P holds every step
            CHECK(w3::aoh_str_bytes(L[b]) >= w3::AOH_STR_PAD + ((uint64_t)L[b] + 31) / 32 * 4 + 4 && w3::aoh_p_steps(L[b]) >= L[b], "%s: block %u sizes", what, b);
            s += w3::aoh_str_bytes(L[b]); ps += w3::aoh_p_steps(L[b]);
        }
        CHECK(bt.str_bytes == s && bt.p_steps == ps, "%s: batch %zu totals", what, k);
        CHECK(w3::AohPlan::bytes(s, ps) <= budget, "%s: batch %zu takes %llu bytes, budget %llu", what, k, (unsigned long long)w3::AohPlan::bytes(s, ps), (unsigned long long)budget);
        next = bt.first + bt.count;
        if (next < nb)   // closed for a reason: the next block would not have fitted, or the cap
            CHECK((cap && bt.count == cap) || w3::AohPlan::bytes(s + w3::aoh_str_bytes(L[next]), ps + w3::aoh_p_steps(L[next])) > budget, "%s: batch %zu closed early", what, k);
        max_s = std::max(max_s, s); max_p = std::max(max_p, ps);
    }
    CHECK(next == nb, "%s: the batches end at block %u of %zu", what, next, nb);
    for (size_t b = 0; b < nb; b++) CHECK(seen[b] == 1, "%s: block %zu is in %d batches", what, b, seen[b]);
    CHECK(p.max_str_bytes == max_s && p.max_p_steps == max_p, "%s: maxima", what);
}

static void plan_cases(uint64_t seed, int rounds) {
    std::mt19937_64 rng(seed);
    for (int r = 0; r < rounds; r++) {
        const size_t nb = rng() % 60;
        std::vector<uint32_t> L(nb);
        for (auto &l : L) l = rng() % 4 == 0 ? (uint32_t)(rng() % 3) * 64u : (uint32_t)(rng() % 300000);
        uint64_t total = 0;
        for (uint32_t l : L) total += w3::AohPlan::bytes(w3::aoh_str_bytes(l), w3::aoh_p_steps(l));
        const uint64_t budgets[] = {~0ull, total, total / 2 + 1, total / 7 + 1, 700000, 1000};
        for (uint64_t budget : budgets)
            for (uint32_t cap : {0u, 1u, 3u, 64u}) check_plan(L, budget, cap, "random");
    }
    check_plan({}, 1000, 0, "no blocks");
    check_plan({0, 0, 0}, 1000, 0, "empty blocks");
    check_plan({0, 1, 63, 64, 65}, ~0ull, 0, "short blocks");
    // offsets are 64-bit: five blocks of nearly 2^32 bits each in one batch — P offsets beyond 2^33 steps
    {
        const std::vector<uint32_t> L(5, 0xFFFFFF01u);
        check_plan(L, ~0ull, 0, "2^32-bit blocks");
        w3::AohPlan p;
        CHECK(w3::aoh_plan(L.data(), L.size(), ~0ull, 0, p) && p.batches.size() == 1, "2^32-bit blocks: one batch");
        CHECK(p.p_off[4] == 4ull * 0xFFFFFF40ull && p.p_off[4] > (1ull << 33), "2^32-bit blocks: p_off[4] = %llu", (unsigned long long)p.p_off[4]);
        CHECK(p.str_off[4] > (1ull << 30) && p.batches[0].p_steps == 5ull * 0xFFFFFF40ull, "2^32-bit blocks: totals");
        check_plan(L, 3ull * w3::AohPlan::bytes(w3::aoh_str_bytes(L[0]), w3::aoh_p_steps(L[0])), 0, "2^32-bit blocks, three per batch");
    }
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 400;
    string_cases(20240607, rounds);
    plan_cases(77, rounds);
    std::printf("aoh plan ok: %lu checks\n", g_checks);
    return 0;
}
