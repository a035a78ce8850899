// Host harness for widen_to_whole_blocks of weath3rb0i_amd/csrc/w3_ranges.h (tests/test_ranges_plan_whole.py): the plan of a CHECKED
// ranges call, compiled for the CPU and checked over seeded random cases and the edge cases of ranges_plan.cpp.  Every touched block
// must be decoded to its true end (the short last block included), the staging layout must be the exclusive scan, the jobs a
// longest-first permutation, the simulated decode + gather must give the requested slices, and blocks, out_len and the pieces' dst and
// len must be those of the unwidened plan.
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

static void run_case(const std::vector<uint8_t> &data, uint64_t bs, const std::vector<w3_range> &rs, const char *what) {
    const uint64_t n = data.size();
    w3::RangePlan p0, p;
    CHECK(w3::plan_ranges(n, bs, nblocks_of(n, bs), rs.data(), rs.size(), p0) == W3_OK, "%s: plan", what);
    p = p0;
    w3::widen_to_whole_blocks(p, n, bs);
    CHECK(p.blocks == p0.blocks && p.out_len == p0.out_len, "%s: blocks / out_len changed", what);
    CHECK(p.blen.size() == p.blocks.size() && p.bdst.size() == p.blocks.size() && p.jobs.size() == p.blocks.size(), "%s: sizes", what);
    uint64_t scan = 0;
    for (size_t k = 0; k < p.blocks.size(); k++) {
        const uint64_t start = (uint64_t)p.blocks[k] * bs, true_len = std::min(bs, n - start);
        CHECK(p.blen[k] == true_len, "%s: block %u decoded for %u of %llu bytes", what, p.blocks[k], p.blen[k], (unsigned long long)true_len);
        CHECK(p.blen[k] >= p0.blen[k], "%s: block %u narrowed", what, p.blocks[k]);
        CHECK(p.bdst[k] == scan, "%s: staging offset of block %u", what, p.blocks[k]);
        scan += p.blen[k];
    }
    CHECK(p.staging == scan, "%s: staging size", what);
    for (size_t k = 0; k < p.jobs.size(); k++) {
        const auto &jb = p.jobs[k];
        const size_t at = (size_t)(std::lower_bound(p.blocks.begin(), p.blocks.end(), jb.blk) - p.blocks.begin());
        CHECK(at < p.blocks.size() && p.blocks[at] == jb.blk && p.blen[at] == jb.len && p.bdst[at] == jb.dst, "%s: job %zu", what, k);
        if (k) CHECK(p.jobs[k - 1].len > jb.len || (p.jobs[k - 1].len == jb.len && p.jobs[k - 1].blk < jb.blk), "%s: job order at %zu", what, k);
    }
    const std::vector<w3::RangeJob> cj = w3::compact_jobs(p);
    for (size_t k = 0; k < cj.size(); k++)
        CHECK(cj[k].blk < p.blocks.size() && p.blocks[cj[k].blk] == p.jobs[k].blk && cj[k].len == p.jobs[k].len && cj[k].dst == p.jobs[k].dst,
              "%s: compact job %zu", what, k);
    // simulated decode, gather, compare
    std::vector<uint8_t> staging(p.staging + 1, 0xA5);
    for (const auto &jb : p.jobs) {
        CHECK(jb.dst + jb.len <= p.staging && (uint64_t)jb.blk * bs + jb.len <= n, "%s: job out of bounds", what);
        std::memcpy(staging.data() + jb.dst, data.data() + (uint64_t)jb.blk * bs, jb.len);
    }
    CHECK(p.pieces.size() == rs.size() && p0.pieces.size() == rs.size(), "%s: piece count", what);
    std::vector<uint8_t> out(p.out_len + 1, 0x5A), want;
    for (size_t q = 0; q < rs.size(); q++) {
        const auto &pc = p.pieces[q];
        CHECK(pc.dst == p0.pieces[q].dst && pc.len == p0.pieces[q].len && pc.len == rs[q].len, "%s: piece %zu dst / len changed", what, q);
        CHECK(pc.len == 0 || pc.src + pc.len <= p.staging, "%s: piece %zu past staging", what, q);
        if (pc.len) std::memcpy(out.data() + pc.dst, staging.data() + pc.src, pc.len);
        want.insert(want.end(), data.begin() + (long)rs[q].offset, data.begin() + (long)(rs[q].offset + rs[q].len));
    }
    out.resize(p.out_len);
    CHECK(out == want, "%s: output differs from the slices", what);
    std::vector<uint8_t> o2(p.out_len, 0x5A);
    for (const auto &c : w3::gather_chunks(p, 65536)) std::memcpy(o2.data() + c.dst, staging.data() + c.src, c.len);
    CHECK(o2 == want, "%s: chunks", what);
}

int main(int argc, char **argv) {
    const int n_random = argc > 1 ? std::atoi(argv[1]) : 4000;
    std::mt19937_64 rng(20261018);
    auto make = [&](uint64_t n) {
        std::vector<uint8_t> d(n);
        for (auto &c : d) c = (uint8_t)rng();
        return d;
    };
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
            run_case(d, bs, {{0, 1}}, "first byte");
            run_case(d, bs, {{n - 1, 1}, {n - std::min<uint64_t>(n, 3), std::min<uint64_t>(n, 3)}}, "range ending at orig_len");
            const uint64_t last0 = (nblocks_of(n, bs) - 1) * bs;
            run_case(d, bs, {{last0, 1}}, "first byte of the short last block");
            run_case(d, bs, {{last0, n - last0}, {last0 + (n - last0) / 2, (n - last0) - (n - last0) / 2}}, "inside the short last block");
            run_case(d, bs, {{n / 2, 0}, {0, 0}, {n, 0}}, "zero-length ranges only");
            run_case(d, bs, {{n / 3, n / 2}, {n / 3, n / 2}, {n / 4, n / 2}, {0, 1}, {n / 2, n - n / 2}}, "duplicate, overlapping, unsorted");
            std::vector<w3_range> many;
            const uint64_t b0 = (nblocks_of(n, bs) / 2) * bs, bl = std::min(bs, n - b0);
            for (int k = 0; k < 50; k++) { const uint64_t o = b0 + rng() % bl; many.push_back({o, rng() % (b0 + bl - o + 1)}); }
            run_case(d, bs, many, "many ranges inside one block");
        }
    }
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
            if (k && rng() % 5 == 0) rs.push_back(rs[rng() % rs.size()]);
        }
        run_case(d, bs, rs, "random");
    }
    std::printf("whole-block plan ok: %lu checks\n", g_checks);
    return 0;
}
