// w3_ranges.h — the plan of a random-access decode (w3_decode_ranges / w3_decode_ranges_device), in plain C++ so that the host can run it
// too: tests/test_ranges_plan.py compiles this file with g++ and checks the plan against a simulated decode over seeded random cases.
//
// Blocks are coded independently (fresh model + coder each, byte-aligned streams), so a byte range needs only the blocks it touches, and
// each of those only up to the last requested byte in it: the arithmetic decoder never has to reach the end of a stream.  The plan:
//   blocks  the distinct blocks the ranges touch, ascending; block k is decoded for blen[k] = (largest range end inside it) - block start
//           bytes into a staging buffer at bdst[k] = the exclusive scan of blen.  Every block a range passes through but its last one is
//           decoded to the block end, so a range that spans several blocks is one contiguous stretch of the staging buffer.
//   jobs    one per distinct block, longest first (ties by block index): a wavefront runs as long as its longest lane, and the decode
//           kernels give consecutive jobs to the lanes of one wavefront (64 blocks per wave in the lane kernels, 4 in k_decode_spec).
//   pieces  one per range {src in staging, dst in the packed output, len}: the output is the ranges concatenated in request order
//           (overlapping, duplicate, unsorted and zero-length ranges are all valid).
// The host-buffer variant copies only the selected streams (blocks[k] in order) and hands the decoder the compact length table
// {block_lens[blocks[k]]}; its jobs then name a stream by its index k in that table (compact_jobs).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/w3hip.h"

namespace w3 {

// a decode job: the lane that takes it decodes stream `blk` (index into the length table) for `len` bytes to staging + dst.
// The same layout as DecodeJob of the decode kernels (w3_generic.h).
struct RangeJob { uint32_t blk; uint32_t len; uint64_t dst; };
struct RangePiece { uint64_t src, dst, len; };

struct RangePlan {
    std::vector<uint32_t> blocks;     // distinct blocks touched, ascending
    std::vector<uint32_t> blen;       // bytes of blocks[k] to decode
    std::vector<uint64_t> bdst;       // staging offset of blocks[k]
    uint64_t staging = 0;             // staging bytes (sum of blen)
    std::vector<RangeJob> jobs;       // blk = block index, longest first, ties by block index
    std::vector<RangePiece> pieces;   // one per range, in request order
    uint64_t out_len = 0;             // sum of the range lengths
};

// W3_OK, or W3_E_INVALID: a block count that does not match orig_len / block_size (checked first), a range past orig_len (u64 wrap
// included), a block size the jobs cannot describe (0, or above 2^32 - 1), or more blocks than a job can name (2^32).
inline int plan_ranges(uint64_t orig_len, uint64_t block_size, uint64_t nblocks, const w3_range *ranges, size_t n_ranges, RangePlan &p) {
    p = RangePlan();
    if (block_size == 0 || block_size > 0xFFFFFFFFull) return W3_E_INVALID;
    if (nblocks != orig_len / block_size + (orig_len % block_size != 0)) return W3_E_INVALID;
    if (nblocks > 0xFFFFFFFFull) return W3_E_INVALID;
    if (n_ranges && !ranges) return W3_E_INVALID;
    for (size_t i = 0; i < n_ranges; i++)
        if (ranges[i].len > orig_len || ranges[i].offset > orig_len - ranges[i].len) return W3_E_INVALID;
    // interior blocks (decoded to the block end) as half-open block intervals, and each range's last block with its end in that block
    std::vector<std::pair<uint64_t, uint64_t>> full;
    std::vector<std::pair<uint64_t, uint64_t>> tail;
    full.reserve(n_ranges); tail.reserve(n_ranges);
    for (size_t i = 0; i < n_ranges; i++) {
        const w3_range &r = ranges[i];
        if (!r.len) continue;
        const uint64_t f = r.offset / block_size, l = (r.offset + r.len - 1) / block_size;
        if (f < l) full.emplace_back(f, l);
        tail.emplace_back(l, r.offset + r.len - l * block_size);
    }
    std::sort(full.begin(), full.end());
    std::sort(tail.begin(), tail.end());
    std::vector<std::pair<uint64_t, uint64_t>> merged;   // disjoint, ascending
    for (const auto &iv : full) {
        if (!merged.empty() && iv.first <= merged.back().second) merged.back().second = std::max(merged.back().second, iv.second);
        else merged.push_back(iv);
    }
    size_t i = 0, j = 0;
    auto emit = [&](uint64_t b, uint64_t len) {
        if (!p.blocks.empty() && p.blocks.back() == (uint32_t)b) { p.blen.back() = std::max<uint32_t>(p.blen.back(), (uint32_t)len); return; }
        p.blocks.push_back((uint32_t)b); p.blen.push_back((uint32_t)len);
    };
    while (i < merged.size() || j < tail.size()) {
        if (i < merged.size() && (j == tail.size() || merged[i].first <= tail[j].first)) {
            for (uint64_t b = merged[i].first; b < merged[i].second; b++) emit(b, block_size);   // (an interior block is never the short last one)
            while (j < tail.size() && tail[j].first < merged[i].second) j++;                   // (its tails end inside the block: shorter)
            i++;
        } else {
            emit(tail[j].first, tail[j].second);
            j++;
        }
    }
    const size_t nd = p.blocks.size();
    p.bdst.resize(nd);
    for (size_t k = 0; k < nd; k++) { p.bdst[k] = p.staging; p.staging += p.blen[k]; }
    p.jobs.resize(nd);
    for (size_t k = 0; k < nd; k++) p.jobs[k] = RangeJob{p.blocks[k], p.blen[k], p.bdst[k]};
    std::stable_sort(p.jobs.begin(), p.jobs.end(), [](const RangeJob &a, const RangeJob &b) { return a.len > b.len; });   // (ties keep block order)
    p.pieces.resize(n_ranges);
    for (size_t q = 0; q < n_ranges; q++) {
        const w3_range &r = ranges[q];
        RangePiece pc{0, p.out_len, r.len};
        if (r.len) {
            const uint64_t f = r.offset / block_size;
            const size_t k = (size_t)(std::lower_bound(p.blocks.begin(), p.blocks.end(), (uint32_t)f) - p.blocks.begin());
            pc.src = p.bdst[k] + (r.offset - f * block_size);
        }
        p.pieces[q] = pc;
        p.out_len += r.len;
    }
    return W3_OK;
}

// The plan of a CHECKED ranges call (the *_checked entry points): a CRC vouches for a whole block, never for a prefix, so every touched
// block is decoded to its end (the short last block: to orig_len).  blen, bdst, staging and jobs are recomputed, and every piece keeps its
// offset inside its first block; blocks, out_len and the pieces' dst and len stay as plan_ranges left them.  A range that runs through
// several blocks is still one contiguous stretch of the staging buffer: every block before the input's last one is block_size long.
inline void widen_to_whole_blocks(RangePlan &p, uint64_t orig_len, uint64_t block_size) {
    const size_t nd = p.blocks.size();
    const std::vector<uint64_t> old_dst(p.bdst);
    p.staging = 0;
    for (size_t k = 0; k < nd; k++) {
        const uint64_t start = (uint64_t)p.blocks[k] * block_size;
        p.blen[k] = (uint32_t)std::min(block_size, orig_len - start);
        p.bdst[k] = p.staging;
        p.staging += p.blen[k];
    }
    for (size_t k = 0; k < nd; k++) p.jobs[k] = RangeJob{p.blocks[k], p.blen[k], p.bdst[k]};
    std::stable_sort(p.jobs.begin(), p.jobs.end(), [](const RangeJob &a, const RangeJob &b) { return a.len > b.len; });   // (ties keep block order)
    for (auto &pc : p.pieces) {
        if (!pc.len) continue;
        const size_t k = (size_t)(std::upper_bound(old_dst.begin(), old_dst.end(), pc.src) - old_dst.begin()) - 1;   // (the block the piece starts in)
        pc.src = p.bdst[k] + (pc.src - old_dst[k]);
    }
}

// the host-buffer variant's jobs: blk = the stream's index in the compact length table (the order of p.blocks)
inline std::vector<RangeJob> compact_jobs(const RangePlan &p) {
    std::vector<RangeJob> out(p.jobs);
    for (auto &jb : out) jb.blk = (uint32_t)(std::lower_bound(p.blocks.begin(), p.blocks.end(), jb.blk) - p.blocks.begin());
    return out;
}

// the gather's work list: every piece cut into chunks of at most `chunk` bytes (one workgroup each); zero-length pieces drop out
inline std::vector<RangePiece> gather_chunks(const RangePlan &p, uint64_t chunk) {
    std::vector<RangePiece> out;
    for (const auto &pc : p.pieces)
        for (uint64_t o = 0; o < pc.len; o += chunk) out.push_back(RangePiece{pc.src + o, pc.dst + o, std::min(chunk, pc.len - o)});
    return out;
}

}  // namespace w3
