// Host harness for weath3rb0i_amd/csrc/w3_tables_plan.h (tests/test_tables_plan.py), compiled for the CPU.
//   Table forms: the five places of the host code that decide a Counter table's form (layout_generic, w3_sweep_ordern_device, aoh_launch,
//   aoh_wave_table, the LEAF_WAVE branch of twophase_predict) are restated here twice — as they stood before counter_table existed
//   (ref_*: each with its own copy of the rule, its own floor and tail) and as they call counter_table now (site_*) — and every value
//   they derive is compared on seeded random (bits, block size / steps), on every exact tie and on the ends of the ranges.
//   Plans: plan_cfg_batches and lanes_per_batch against the planning loops aoh_launch and aoh_spec_launch had (ref_plan,
//   ref_spec_lanes), under every budget the halving retry would try, and on their own: every (configuration, block) exactly once,
//   batches within the budget and the lane cap, table areas one behind the other, whole wavefronts, false exactly when one table
//   exceeds the budget, 64-bit products.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../weath3rb0i_amd/csrc/w3_tables_plan.h"

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
typedef unsigned long long ull;

// ---------------------------------------------------------------------------------------------------------------------------------
// the rule as the five sites spelled it out
// ---------------------------------------------------------------------------------------------------------------------------------
static uint64_t ref_next_pow2(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
struct Form { uint64_t use_hash, mask_or_slots, bytes; };   // what a site derives: the form, its hash mask / slot count, the table's bytes
static bool same(const Form &a, const Form &b) { return a.use_hash == b.use_hash && a.mask_or_slots == b.mask_or_slots && a.bytes == b.bytes; }

static Form ref_layout_generic(uint32_t bits, uint64_t block_size) {
    const uint64_t steps = (uint64_t)block_size * 8;
    const uint64_t hash_slots = std::max<uint64_t>(1024, ref_next_pow2(2 * steps));
    const uint64_t hash_bytes = hash_slots * 8;
    Form f{0, 0, 0};
    const uint64_t direct_bytes = 4ull << bits;
    if (direct_bytes <= hash_bytes) { f.use_hash = 0; f.bytes = direct_bytes; }
    else { f.use_hash = 1; f.mask_or_slots = (uint32_t)(hash_slots - 1); f.bytes = hash_bytes; }
    return f;
}
static Form ref_sweep_ordern(uint32_t bits, uint64_t block_size) {
    const uint64_t steps = (uint64_t)block_size * 8;
    const uint64_t hash_slots = std::max<uint64_t>(1024, ref_next_pow2(2 * steps)), hash_bytes = hash_slots * 8;
    const uint64_t direct = 4ull << bits;
    const bool hashed = direct > hash_bytes;
    const uint64_t stride = hashed ? hash_bytes : std::max<uint64_t>(direct, 16);
    return Form{hashed, (uint32_t)(hash_slots - 1), stride};
}
static Form ref_aoh_launch(uint32_t ctx_bits, uint64_t steps) {
    const uint64_t slots = std::max<uint64_t>(1024, ref_next_pow2(2 * steps)), hash_bytes = slots * 8, direct = 4ull << ctx_bits;
    const bool use_hash = direct > hash_bytes;
    return Form{use_hash, (uint32_t)(slots - 1), use_hash ? hash_bytes : std::max<uint64_t>(direct, 16)};
}
static Form ref_aoh_wave_table(uint32_t ctx_bits, uint64_t max_l) {
    const uint64_t slots = std::max<uint64_t>(1024, ref_next_pow2(2 * max_l)), hash_bytes = 8 * slots + 16, direct = std::max<uint64_t>(4ull << ctx_bits, 16);
    const bool use_hash = direct > hash_bytes;
    return Form{use_hash, slots, use_hash ? hash_bytes : direct};
}
static Form ref_leaf_wave(uint32_t bits, uint64_t block_size) {
    const uint64_t hash_slots = std::max<uint64_t>(1024, ref_next_pow2(16ull * block_size));
    const uint64_t hash_bytes = 8ull * hash_slots + 16ull, direct_bytes = std::max<uint64_t>(4ull << bits, 16ull);
    const uint32_t use_hash = (bits >= 32 || direct_bytes > hash_bytes) ? 1u : 0u;
    return Form{use_hash, (uint32_t)hash_slots, use_hash ? hash_bytes : direct_bytes};
}

// ... and as the sites call counter_table
static Form site_layout_generic(uint32_t bits, uint64_t block_size) {
    const w3::CounterTable t = w3::counter_table(bits, (uint64_t)block_size * 8);
    return Form{t.use_hash, t.use_hash ? (uint32_t)(t.slots - 1) : 0u, t.use_hash ? t.hash_bytes : t.direct_bytes};
}
static Form site_sweep_ordern(uint32_t bits, uint64_t block_size) {
    const w3::CounterTable t = w3::counter_table(bits, (uint64_t)block_size * 8);
    return Form{t.use_hash, (uint32_t)(t.slots - 1), t.use_hash ? t.hash_bytes : std::max<uint64_t>(t.direct_bytes, 16)};
}
static Form site_aoh_launch(uint32_t ctx_bits, uint64_t steps) {
    const w3::CounterTable t = w3::counter_table(ctx_bits, steps);
    return Form{t.use_hash, (uint32_t)(t.slots - 1), t.use_hash ? t.hash_bytes : std::max<uint64_t>(t.direct_bytes, 16)};
}
static Form site_aoh_wave_table(uint32_t ctx_bits, uint64_t max_l) {
    const w3::CounterTable c = w3::counter_table(ctx_bits, max_l);
    return Form{c.use_hash, c.slots, c.use_hash ? c.hash_bytes + 16 : std::max<uint64_t>(c.direct_bytes, 16)};
}
static Form site_leaf_wave(uint32_t bits, uint64_t block_size) {
    const w3::CounterTable ct = w3::counter_table(bits, 8ull * block_size);
    const uint64_t hash_bytes = ct.hash_bytes + 16ull, direct_bytes = std::max<uint64_t>(ct.direct_bytes, 16ull);
    const uint32_t use_hash = (bits >= 32 || ct.use_hash) ? 1u : 0u;
    return Form{use_hash, (uint32_t)ct.slots, use_hash ? hash_bytes : direct_bytes};
}

static void check_forms(uint32_t bits, uint64_t block_size, uint64_t steps) {
    CHECK(same(ref_layout_generic(bits, block_size), site_layout_generic(bits, block_size)), "layout_generic: bits %u block_size %llu", bits, (ull)block_size);
    CHECK(same(ref_sweep_ordern(bits, block_size), site_sweep_ordern(bits, block_size)), "w3_sweep_ordern_device: bits %u block_size %llu", bits, (ull)block_size);
    CHECK(same(ref_leaf_wave(bits, block_size), site_leaf_wave(bits, block_size)), "LEAF_WAVE: bits %u block_size %llu", bits, (ull)block_size);
    CHECK(same(ref_aoh_launch(bits, steps), site_aoh_launch(bits, steps)), "aoh_launch: bits %u steps %llu", bits, (ull)steps);
    CHECK(same(ref_aoh_wave_table(bits, steps), site_aoh_wave_table(bits, steps)), "aoh_wave_table: bits %u steps %llu", bits, (ull)steps);
    // the rule on its own: the smaller form, direct on a tie; at most half the map's slots fill
    const w3::CounterTable t = w3::counter_table(bits, steps);
    CHECK(t.direct_bytes == 4ull << bits && t.hash_bytes == 8 * t.slots && t.slots >= 1024 && (t.slots & (t.slots - 1)) == 0, "bits %u steps %llu: sizes", bits, (ull)steps);
    CHECK(t.slots >= 2 * steps && (t.slots == 1024 || t.slots < 4 * steps), "bits %u steps %llu: %llu slots", bits, (ull)steps, (ull)t.slots);
    CHECK(t.use_hash == (t.hash_bytes < t.direct_bytes), "bits %u steps %llu: form", bits, (ull)steps);
}

// up to 2^hi, every magnitude from 2^lo on as likely as any other
static uint64_t log_uniform(std::mt19937_64 &rng, unsigned lo, unsigned hi) {
    const unsigned e = lo + (unsigned)(rng() % (hi - lo + 1));
    return e == 0 ? 1 : (1ull << e) - rng() % (1ull << (e - 1));
}

static void form_cases(uint64_t seed, int rounds) {
    std::mt19937_64 rng(seed);
    for (int r = 0; r < rounds * 50; r++) check_forms(1 + (uint32_t)(rng() % 32), log_uniform(rng, 0, 28), log_uniform(rng, 0, 31));
    for (uint32_t bits = 1; bits <= 32; bits++) {
        for (uint64_t v : {1ull, 2ull, 63ull, 64ull, 65ull, 511ull, 512ull, 513ull, 65536ull, (1ull << 28) - 1, 1ull << 28}) check_forms(bits, v, 8 * v);
        check_forms(bits, 1, 0);          // (a call whose every block codes to no bits)
        check_forms(bits, 1, 1ull << 31);
        check_forms(bits, 1, 0xFFFFFFFFull);   // (the largest bit count a block can have)
    }
    // every tie: a map of 2^k slots is as large as the direct table of k + 1 bits — the direct table it is
    for (uint32_t k = 10; k <= 31; k++)
        for (uint64_t steps : {k == 10 ? 1ull : (1ull << (k - 2)) + 1, 1ull << (k - 1)}) {
            const w3::CounterTable t = w3::counter_table(k + 1, steps);
            CHECK(t.slots == 1ull << k && t.direct_bytes == t.hash_bytes && !t.use_hash, "tie at %u bits, %llu steps", k + 1, (ull)steps);
            CHECK(w3::counter_table(k + 2, steps).use_hash && !w3::counter_table(k, steps).use_hash, "beside the tie at %u bits", k + 1);
            if (steps % 8 == 0) check_forms(k + 1, steps / 8, steps);
            else check_forms(k + 1, 1, steps);
        }
    for (uint64_t v : {0ull, 1ull, 2ull, 3ull, 4ull, 5ull, 1023ull, 1024ull, 1025ull, (1ull << 33) - 1, 1ull << 33, (1ull << 33) + 1, 1ull << 62})
        CHECK(w3::next_pow2(v) == ref_next_pow2(v) && w3::next_pow2(v) >= v && (v < 2 || w3::next_pow2(v) < 2 * v), "next_pow2(%llu)", (ull)v);
    for (uint64_t f : {0ull, 1000ull, 1ull << 30, 255ull << 30, 266ull << 30, 288ull << 30, 1ull << 40})
        for (uint64_t h : {0ull, 256ull, 10ull << 30, 150ull << 30})
            CHECK(w3::sweep_budget(f, h) == std::min<uint64_t>((uint64_t)(f + h) * 3 / 4, 200ull << 30), "sweep_budget(%llu, %llu)", (ull)f, (ull)h);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the planning loops as aoh_launch and aoh_spec_launch had them
// ---------------------------------------------------------------------------------------------------------------------------------
struct RefCfg { uint64_t stride, base; };
struct RefBatch { size_t c0, c1; uint32_t first_block, n_lanes; uint64_t used; };
static bool ref_plan(std::vector<RefCfg> &cfg, uint32_t nb, uint64_t budget, uint32_t max_lanes, std::vector<RefBatch> &plan, uint64_t &need_out) {
    const size_t ncfg = cfg.size();
    plan.clear();
    uint64_t need = 0;
    bool fits = true;
    for (size_t c0 = 0; c0 < ncfg && fits;) {
        if (cfg[c0].stride * nb <= budget && (!max_lanes || nb <= max_lanes)) {   // whole configurations
            uint64_t used = 0;
            size_t c1 = c0;
            for (; c1 < ncfg && used + cfg[c1].stride * nb <= budget; c1++) { cfg[c1].base = used; used += cfg[c1].stride * nb; }
            plan.push_back({c0, c1, 0u, nb, used});
            need = std::max(need, used);
            c0 = c1;
        } else {                                                   // one configuration, batches of blocks
            uint64_t lanes = budget / cfg[c0].stride;
            if (max_lanes) lanes = std::min<uint64_t>(lanes, max_lanes);
            if (lanes >= 64) lanes = lanes / 64 * 64;
            if (lanes == 0) { fits = false; break; }
            cfg[c0].base = 0;
            for (uint32_t b0 = 0; b0 < nb; b0 += (uint32_t)lanes) {
                const uint32_t cnt = (uint32_t)std::min<uint64_t>(lanes, nb - b0);
                plan.push_back({c0, c0 + 1, b0, cnt, cfg[c0].stride * cnt});
                need = std::max(need, cfg[c0].stride * cnt);
            }
            c0++;
        }
    }
    need_out = need;
    return fits;
}
static uint64_t ref_spec_lanes(uint64_t budget, uint64_t stride, uint32_t nl, uint32_t aoh_batch_blocks) {
    uint64_t lanes = std::min<uint64_t>(budget / stride, nl);
    if (aoh_batch_blocks) lanes = std::min<uint64_t>(lanes, aoh_batch_blocks);
    if (lanes >= 4) lanes = lanes / 4 * 4;
    return lanes;
}

static void check_plan(const std::vector<uint64_t> &strides, uint32_t nb, uint64_t budget, uint32_t max_lanes, const char *what) {
    const size_t ncfg = strides.size();
    std::vector<w3::CfgBatch> plan;
    std::vector<uint64_t> base(ncfg, ~0ull);
    uint64_t need = 0;
    const bool ok = w3::plan_cfg_batches(strides.data(), ncfg, nb, budget, max_lanes, plan, base.data(), need);
    const uint64_t widest = *std::max_element(strides.begin(), strides.end());
    CHECK(ok == (widest <= budget), "%s: plan %d, widest table %llu, budget %llu", what, (int)ok, (ull)widest, (ull)budget);
    std::vector<RefCfg> rc(ncfg);
    for (size_t c = 0; c < ncfg; c++) rc[c] = RefCfg{strides[c], ~0ull};
    std::vector<RefBatch> rp;
    uint64_t rneed = 0;
    CHECK(ref_plan(rc, nb, budget, max_lanes, rp, rneed) == ok, "%s: the loop of aoh_launch says %d", what, (int)!ok);
    if (!ok) return;
    CHECK(need == rneed && plan.size() == rp.size(), "%s: need %llu (%llu), %zu batches (%zu)", what, (ull)need, (ull)rneed, plan.size(), rp.size());
    for (size_t c = 0; c < ncfg; c++) CHECK(base[c] == rc[c].base, "%s: base of configuration %zu", what, c);
    std::vector<uint32_t> next(ncfg, 0);   // per configuration: the first block no batch has taken yet
    uint64_t largest = 0;
    for (size_t k = 0; k < plan.size(); k++) {
        const w3::CfgBatch &bt = plan[k];
        CHECK(bt.c0 == rp[k].c0 && bt.c1 == rp[k].c1 && bt.first_block == rp[k].first_block && bt.n_lanes == rp[k].n_lanes && bt.used == rp[k].used, "%s: batch %zu", what, k);
        CHECK(bt.c0 < bt.c1 && bt.c1 <= ncfg && bt.n_lanes > 0, "%s: batch %zu is empty", what, k);
        CHECK(bt.used <= budget, "%s: batch %zu takes %llu bytes, budget %llu", what, k, (ull)bt.used, (ull)budget);
        CHECK(!max_lanes || bt.n_lanes <= max_lanes, "%s: batch %zu has %u lanes, cap %u", what, k, bt.n_lanes, max_lanes);
        const bool whole = bt.first_block == 0 && bt.n_lanes == nb;
        CHECK(whole || bt.c1 == bt.c0 + 1, "%s: batch %zu holds parts of several configurations", what, k);
        uint64_t off = 0;
        for (size_t c = bt.c0; c < bt.c1; c++) {
            CHECK(bt.first_block == next[c], "%s: batch %zu starts configuration %zu at block %u, want %u", what, k, c, bt.first_block, next[c]);
            CHECK((uint64_t)next[c] + bt.n_lanes <= nb, "%s: batch %zu runs past the last block", what, k);
            next[c] += bt.n_lanes;
            // table areas: one behind the other from 0 (k_aoh: base + stride x (block - first_block))
            CHECK(base[c] == off, "%s: batch %zu: configuration %zu at %llu, want %llu", what, k, c, (ull)base[c], (ull)off);
            off += strides[c] * bt.n_lanes;
        }
        CHECK(off == bt.used, "%s: batch %zu: used %llu, its tables take %llu", what, k, (ull)bt.used, (ull)off);
        // whole wavefronts, but for a configuration's last batch
        if (!whole && next[bt.c0] < nb && bt.n_lanes >= 64) CHECK(bt.n_lanes % 64 == 0, "%s: batch %zu has %u lanes", what, k, bt.n_lanes);
        largest = std::max(largest, bt.used);
    }
    for (size_t c = 0; c < ncfg; c++) CHECK(next[c] == nb, "%s: configuration %zu: blocks up to %u of %u", what, c, next[c], nb);
    CHECK(need == largest, "%s: need", what);
}

static void check_spec(uint64_t budget, uint64_t stride, uint32_t nl, uint32_t cap, const char *what) {
    const uint64_t per = w3::lanes_per_batch(budget, stride, nl, cap, 4);
    CHECK(per == ref_spec_lanes(budget, stride, nl, cap), "%s: %llu jobs per batch, aoh_spec_launch took %llu", what, (ull)per, (ull)ref_spec_lanes(budget, stride, nl, cap));
    CHECK((per == 0) == (stride > budget), "%s: %llu jobs, stride %llu, budget %llu", what, (ull)per, (ull)stride, (ull)budget);
    CHECK(per <= nl && (!cap || per <= cap) && per * stride <= budget, "%s: %llu jobs per batch", what, (ull)per);
    CHECK(per < 4 || per % 4 == 0, "%s: %llu jobs per batch", what, (ull)per);
    CHECK(per + 4 > std::min<uint64_t>(std::min<uint64_t>(budget / stride, nl), cap ? cap : ~0ull), "%s: %llu jobs per batch where more fit", what, (ull)per);
}

static const uint32_t MAX_LANES[] = {0, 3, 4, 64, 100};

static void plan_cases(uint64_t seed, int rounds) {
    std::mt19937_64 rng(seed);
    for (int r = 0; r < rounds; r++) {
        // (many blocks with few configurations, many configurations with fewer blocks: a batch of blocks holds one configuration, and
        // the tightest budgets below give a batch per block)
        const bool many_blocks = r % 8 == 0;
        const size_t ncfg = 1 + rng() % (many_blocks ? 3 : 40);
        const uint32_t nb = many_blocks ? 1 + (uint32_t)(rng() % 70000) : (uint32_t)log_uniform(rng, 0, 11);
        std::vector<uint64_t> strides(ncfg);
        uint64_t total = 0;
        for (auto &s : strides) {   // (aoh_launch's strides)
            const w3::CounterTable t = w3::counter_table(1 + (uint32_t)(rng() % 32), log_uniform(rng, 0, 31));
            s = t.use_hash ? t.hash_bytes : std::max<uint64_t>(t.direct_bytes, 16);
            total += s * nb;
        }
        const uint64_t widest = *std::max_element(strides.begin(), strides.end());
        const uint64_t budgets[] = {log_uniform(rng, 10, 37), 200ull << 30, total, total / 3 + 1, widest * nb, widest, widest - 1, 64 * widest + 1};
        for (uint64_t b0 : budgets)
            for (uint64_t budget = std::min<uint64_t>(b0, 200ull << 30), h = 0; h < 3 && budget > 0; budget /= 2, h++)   // (the retry halves)
                for (uint32_t ml : MAX_LANES) {
                    check_plan(strides, nb, budget, ml, "random");
                    check_spec(budget, strides[0], nb, ml, "random");
                }
    }
    // products beyond 2^32: 16 GiB tables x 2^16 lanes, twelve of them per batch under 200 GiB
    {
        const std::vector<uint64_t> big(2, 16ull << 30);
        for (uint32_t ml : MAX_LANES) check_plan(big, 1u << 16, 200ull << 30, ml, "16 GiB x 2^16");
        std::vector<w3::CfgBatch> plan;
        uint64_t base[2], need = 0;
        CHECK(w3::plan_cfg_batches(big.data(), 2, 1u << 16, 200ull << 30, 0, plan, base, need), "16 GiB x 2^16: fits");
        CHECK(need == 12 * (16ull << 30) && plan.size() == 2 * 5462 && plan[5461].first_block == 5461 * 12 && plan[5461].n_lanes == 4, "16 GiB x 2^16: %zu batches", plan.size());
        check_plan(big, 1u << 16, (16ull << 30) - 1, 0, "16 GiB x 2^16, a budget below one table");
        check_spec(200ull << 30, 8ull << 30, 1u << 16, 0, "8 GiB x 2^16 jobs");
        check_plan({1ull << 20, 16, 1ull << 30, 16, 16}, 70000, 200ull << 30, 0, "wide and narrow");
        check_plan(std::vector<uint64_t>(40, 1ull << 16), 70000, 200ull << 30, 64, "40 x 70,000");
        check_plan({16, 16, 16}, 70000, 70000 * 32, 0, "two of three fit");
        check_plan({4096}, 129, 4096 * 128, 0, "one block over");
        check_plan({4096}, 1, 4096, 3, "one block");
    }
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 400;
    form_cases(20250118, rounds);
    plan_cases(91, rounds);
    std::printf("tables plan ok: %lu checks\n", g_checks);
    return 0;
}
