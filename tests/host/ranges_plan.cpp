// Host harness for weath3rb0i_amd/csrc/w3_ranges.h (tests/test_ranges_plan.py): the plan of w3_decode_ranges, compiled for the CPU and
// checked over seeded random cases and the edge cases by SIMULATING the decode — every job copies data[b * bs, b * bs + len) to its
// staging offset, the pieces are applied, and the result must be the requested slices concatenated.  Also checked: the blocks are
// distinct and ascending, each is decoded exactly to the largest range end inside it, the staging offsets are the exclusive scan, the
// jobs run longest first (ties by block), and the host variant's compact stream selection names exactly the selected streams.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../weath3rb0i_amd/csrc/w3_ranges.h"

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

static uint64_t nblocks_of(uint64_t n, uint64_t bs) { return (n + bs - 1) / bs; }

// one valid case: plan, simulate, compare, check the plan's invariants
static void run_case(const std::vector<uint8_t> &data, uint64_t bs, const std::vector<w3_range> &rs, const char *what) {
    const uint64_t n = data.size();
    w3::RangePlan p;
    const int rc = w3::plan_ranges(n, bs, nblocks_of(n, bs), rs.data(), rs.size(), p);
    CHECK(rc == W3_OK, "%s: rc %d (n %llu bs %llu)", what, rc, (unsigned long long)n, (unsigned long long)bs);
    // the expected maximum end per block, by brute force
    std::vector<uint64_t> want_len(nblocks_of(n, bs), 0);
    std::vector<char> touched(want_len.size(), 0);
    uint64_t want_out = 0;
    for (const auto &r : rs) {
        want_out += r.len;
        for (uint64_t o = r.offset; o < r.offset + r.len; ) {   // (walk block by block)
            const uint64_t b = o / bs, be = std::min((b + 1) * bs, r.offset + r.len);
            touched[b] = 1;
            want_len[b] = std::max(want_len[b], be - b * bs);
            o = be;
        }
    }
    CHECK(p.out_len == want_out, "%s: out_len", what);
    std::vector<uint32_t> want_blocks;
    for (uint64_t b = 0; b < touched.size(); b++) if (touched[b]) want_blocks.push_back((uint32_t)b);
    CHECK(p.blocks == want_blocks, "%s: distinct blocks (%zu vs %zu)", what, p.blocks.size(), want_blocks.size());
    CHECK(p.blen.size() == p.blocks.size() && p.bdst.size() == p.blocks.size(), "%s: sizes", what);
    uint64_t scan = 0;
    for (size_t k = 0; k < p.blocks.size(); k++) {
        CHECK(p.blen[k] == want_len[p.blocks[k]], "%s: block %u len %u want %llu", what, p.blocks[k], p.blen[k], (unsigned long long)want_len[p.blocks[k]]);
        CHECK(p.bdst[k] == scan, "%s: staging offset", what);
        scan += p.blen[k];
    }
    CHECK(p.staging == scan, "%s: staging size", what);
    // jobs: a permutation of the blocks, longest first, ties by block index
    CHECK(p.jobs.size() == p.blocks.size(), "%s: job count", what);
    for (size_t k = 0; k < p.jobs.size(); k++) {
        const auto &jb = p.jobs[k];
        const size_t at = (size_t)(std::lower_bound(p.blocks.begin(), p.blocks.end(), jb.blk) - p.blocks.begin());
        CHECK(at < p.blocks.size() && p.blocks[at] == jb.blk && p.blen[at] == jb.len && p.bdst[at] == jb.dst, "%s: job %zu", what, k);
        if (k) CHECK(p.jobs[k - 1].len > jb.len || (p.jobs[k - 1].len == jb.len && p.jobs[k - 1].blk < jb.blk), "%s: job order at %zu", what, k);
    }
    // host variant: the compact table names exactly the selected streams, in order
    const std::vector<w3::RangeJob> cj = w3::compact_jobs(p);
    CHECK(cj.size() == p.jobs.size(), "%s: compact job count", what);
    for (size_t k = 0; k < cj.size(); k++)
        CHECK(cj[k].blk < p.blocks.size() && p.blocks[cj[k].blk] == p.jobs[k].blk && cj[k].len == p.jobs[k].len && cj[k].dst == p.jobs[k].dst,
              "%s: compact job %zu", what, k);
    // simulated decode: both job forms fill the staging buffer the same way
    std::vector<uint8_t> staging(p.staging + 1, 0xA5), staging2(p.staging + 1, 0xA5);
    for (const auto &jb : p.jobs) {
        CHECK(jb.dst + jb.len <= p.staging, "%s: job past staging", what);
        CHECK((uint64_t)jb.blk * bs + jb.len <= n, "%s: job past the block", what);
        std::memcpy(staging.data() + jb.dst, data.data() + (uint64_t)jb.blk * bs, jb.len);
    }
    for (const auto &jb : cj) std::memcpy(staging2.data() + jb.dst, data.data() + (uint64_t)p.blocks[jb.blk] * bs, jb.len);
    CHECK(staging == staging2, "%s: compact jobs decode differently", what);
    std::vector<uint8_t> out(p.out_len + 1, 0x5A), want;
    CHECK(p.pieces.size() == rs.size(), "%s: piece count", what);
    uint64_t dst = 0;
    for (size_t q = 0; q < rs.size(); q++) {
        const auto &pc = p.pieces[q];
        CHECK(pc.len == rs[q].len && pc.dst == dst, "%s: piece %zu", what, q);
        CHECK(pc.len == 0 || pc.src + pc.len <= p.staging, "%s: piece %zu past staging", what, q);
        if (pc.len) std::memcpy(out.data() + pc.dst, staging.data() + pc.src, pc.len);
        dst += pc.len;
        want.insert(want.end(), data.begin() + (long)rs[q].offset, data.begin() + (long)(rs[q].offset + rs[q].len));
    }
    out.resize(p.out_len);
    CHECK(out == want, "%s: output differs from the slices", what);
    // the gather's chunks cover every piece exactly, none longer than the chunk size
    for (uint64_t chunk : {1ull, 5ull, 65536ull}) {
        std::vector<uint8_t> o2(p.out_len, 0x5A);
        uint64_t covered = 0;
        for (const auto &c : w3::gather_chunks(p, chunk)) {
            CHECK(c.len >= 1 && c.len <= chunk, "%s: chunk size", what);
            std::memcpy(o2.data() + c.dst, staging.data() + c.src, c.len);
            covered += c.len;
        }
        CHECK(covered == p.out_len && o2 == want, "%s: chunks (chunk %llu)", what, (unsigned long long)chunk);
    }
}

static void expect_invalid(uint64_t n, uint64_t bs, uint64_t nb, const std::vector<w3_range> &rs, const char *what) {
    w3::RangePlan p;
    CHECK(w3::plan_ranges(n, bs, nb, rs.data(), rs.size(), p) == W3_E_INVALID, "%s", what);
}

int main(int argc, char **argv) {
    const int n_random = argc > 1 ? std::atoi(argv[1]) : 4000;
    std::mt19937_64 rng(20261016);
    auto make = [&](uint64_t n) {
        std::vector<uint8_t> d(n);
        for (auto &c : d) c = (uint8_t)rng();
        return d;
    };
    // ---- edge cases ----
    for (uint64_t bs : {1ull, 3ull, 7ull, 4096ull, 65536ull}) {
        run_case({}, bs, {}, "orig_len 0, no ranges");
        run_case({}, bs, {{0, 0}, {0, 0}}, "orig_len 0, zero-length ranges");
        const std::vector<uint8_t> one = make(1);
        run_case(one, bs, {{0, 1}}, "orig_len 1");
        run_case(one, bs, {{1, 0}, {0, 1}, {0, 0}, {0, 1}}, "orig_len 1, zero-length at the end, duplicates");
        for (uint64_t n : {bs * 5, bs * 5 + bs / 2 + 1, bs + 1, 2 * bs - 1}) {
            if (n == 0) continue;
            const std::vector<uint8_t> d = make(n);
            run_case(d, bs, {{0, n}}, "whole input");
            run_case(d, bs, {{n - 1, 1}, {n - std::min<uint64_t>(n, 3), std::min<uint64_t>(n, 3)}}, "range ending at orig_len");
            const uint64_t last0 = (nblocks_of(n, bs) - 1) * bs;
            run_case(d, bs, {{last0, n - last0}, {last0 + (n - last0) / 2, (n - last0) - (n - last0) / 2}}, "inside the short last block");
            run_case(d, bs, {{n / 2, 0}, {0, 0}, {n, 0}}, "zero-length ranges only");
            run_case(d, bs, {{n / 3, n / 2}, {n / 3, n / 2}, {n / 4, n / 2}, {0, 1}, {n / 2, n - n / 2}}, "duplicate, overlapping, unsorted");
            std::vector<w3_range> many;
            const uint64_t b0 = (nblocks_of(n, bs) / 2) * bs, bl = std::min(bs, n - b0);
            for (int k = 0; k < 50; k++) { const uint64_t o = b0 + rng() % bl; many.push_back({o, rng() % (b0 + bl - o + 1)}); }
            run_case(d, bs, many, "many ranges inside one block");
        }
    }
    // ---- invalid arguments ----
    expect_invalid(100, 10, 9, {{0, 1}}, "nblocks too small");
    expect_invalid(100, 10, 11, {{0, 1}}, "nblocks too large");
    expect_invalid(101, 10, 10, {}, "nblocks off by the short block");
    expect_invalid(0, 10, 1, {}, "nblocks for an empty input");
    expect_invalid(100, 10, 9, {{~0ull, 2}}, "nblocks mismatch is checked before the ranges");
    expect_invalid(100, 10, 10, {{0, 101}}, "range past orig_len");
    expect_invalid(100, 10, 10, {{100, 1}}, "range starting at orig_len");
    expect_invalid(100, 10, 10, {{~0ull, 2}}, "offset + len wraps");
    expect_invalid(100, 10, 10, {{1, ~0ull}}, "len wraps");
    expect_invalid(100, 10, 10, {{~0ull - 5, 10}}, "offset + len wraps past 0");
    expect_invalid(100, 0, 0, {}, "block size 0");
    {   // the invalid plan leaves nothing behind: a valid case afterwards on the same plan object
        w3::RangePlan p;
        w3_range r{50, 10};
        CHECK(w3::plan_ranges(100, 10, 10, &r, 1, p) == W3_OK && p.blocks.size() == 1 && p.out_len == 10, "valid after invalid");
        w3_range bad{95, 10};
        CHECK(w3::plan_ranges(100, 10, 10, &bad, 1, p) == W3_E_INVALID && p.blocks.empty() && p.jobs.empty(), "reset on error");
    }
    // ---- seeded random cases ----
    for (int c = 0; c < n_random; c++) {
        const uint64_t bs = (c % 4 == 0) ? 1 + rng() % 4 : (c % 4 == 1) ? 1 + rng() % 64 : (c % 4 == 2) ? 1 + rng() % 1000 : 4096;
        const uint64_t n = rng() % (c % 7 == 0 ? 20000 : 3000);
        const std::vector<uint8_t> d = make(n);
        std::vector<w3_range> rs;
        const int nr = (int)(rng() % 40);
        for (int k = 0; k < nr; k++) {
            const uint64_t o = n ? rng() % (n + 1) : 0;
            uint64_t l;
            switch (rng() % 4) {
            case 0: l = 0; break;
            case 1: l = std::min<uint64_t>(n - o, rng() % 8); break;
            case 2: l = std::min<uint64_t>(n - o, rng() % (2 * bs + 2)); break;
            default: l = n - o ? rng() % (n - o + 1) : 0; break;
            }
            rs.push_back({o, l});
            if (k && rng() % 5 == 0) rs.push_back(rs[rng() % rs.size()]);   // duplicates
        }
        run_case(d, bs, rs, "random");
    }
    std::printf("ranges plan ok: %lu checks\n", g_checks);
    return 0;
}
