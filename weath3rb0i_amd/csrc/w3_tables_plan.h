// w3_tables_plan.h — the host's arithmetic for Counter tables in device memory, plain C++ (no HIP; tests/test_tables_plan.py compiles it with g++): the form
// a lane's table takes, the memory the sweep family's launches may use, and how configurations x blocks are cut into launches that fit.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace w3 {

inline uint64_t next_pow2(uint64_t v) { uint64_t p = 1; while (p < v) p <<= 1; return p; }

// The Counter table of one lane that takes at most `steps` bit-steps under a context of `bits` bits: direct, 4 << bits bytes, or the
// exact map (every context a lane meets has a slot: at most half the slots fill) of max(1024, next_pow2(2 x steps)) 8-byte slots,
// whichever is smaller — direct on a tie.  Floors, tails behind the map and further conditions are the caller's.
struct CounterTable { bool use_hash; uint64_t slots, direct_bytes, hash_bytes; };
inline CounterTable counter_table(uint32_t bits, uint64_t steps) {
    CounterTable t{false, std::max<uint64_t>(1024, next_pow2(2 * steps)), 4ull << bits, 0};
    t.hash_bytes = t.slots * 8;
    t.use_hash = t.direct_bytes > t.hash_bytes;
    return t;
}

// Bytes the tables of one launch of the sweep family (w3_sweep_ordern*, AC over Huffman) may take: three quarters of what is free
// plus what the context holds already, at most 200 GiB.
inline uint64_t sweep_budget(uint64_t free_bytes, uint64_t held_bytes) { return std::min<uint64_t>((free_bytes + held_bytes) * 3 / 4, 200ull << 30); }

// Lanes (tables of `stride` bytes) per batch: what the budget holds, at most `want` and `cap` (0 = no cap), in whole quanta (the lanes
// a wavefront takes) once there is one.  0: one table exceeds the budget.
inline uint64_t lanes_per_batch(uint64_t budget, uint64_t stride, uint64_t want, uint64_t cap, uint64_t quantum) {
    uint64_t lanes = std::min(budget / stride, want);
    if (cap) lanes = std::min(lanes, cap);
    return lanes >= quantum ? lanes / quantum * quantum : lanes;
}

// Launches of configurations [c0, c1) x blocks [first_block, first_block + n_lanes), a lane each; `used` bytes of tables.
struct CfgBatch { size_t c0, c1; uint32_t first_block, n_lanes; uint64_t used; };

// Configurations (lane tables of strides[c] bytes) x nb blocks: as many whole configurations per launch as fit the budget, table
// areas one after the other from base[c]; a configuration that does not fit, or has more blocks than max_lanes (0 = no cap), goes
// alone in batches of blocks (base 0, wavefronts of 64).  need: the largest launch.  false: one lane's table exceeds the budget.
inline bool plan_cfg_batches(const uint64_t *strides, size_t ncfg, uint32_t nb, uint64_t budget, uint32_t max_lanes, std::vector<CfgBatch> &plan,
                             uint64_t *base, uint64_t &need) {
    plan.clear();
    need = 0;
    for (size_t c0 = 0; c0 < ncfg;) {
        if (strides[c0] * nb <= budget && (!max_lanes || nb <= max_lanes)) {
            uint64_t used = 0;
            size_t c1 = c0;
            for (; c1 < ncfg && used + strides[c1] * nb <= budget; c1++) { base[c1] = used; used += strides[c1] * nb; }
            plan.push_back({c0, c1, 0u, nb, used});
            need = std::max(need, used);
            c0 = c1;
        } else {
            const uint64_t lanes = lanes_per_batch(budget, strides[c0], nb, max_lanes, 64);
            if (lanes == 0) return false;
            base[c0] = 0;
            for (uint32_t b0 = 0; b0 < nb; b0 += (uint32_t)lanes) {
                const uint32_t cnt = (uint32_t)std::min<uint64_t>(lanes, nb - b0);
                plan.push_back({c0, c0 + 1, b0, cnt, strides[c0] * cnt});
                need = std::max(need, strides[c0] * cnt);
            }
            c0++;
        }
    }
    return true;
}

}  // namespace w3
