// Host harness of weath3rb0i_amd/csrc/w3_steps_plan.h (tests/test_steps_cpu.py): walks the row kernel's tiles on the CPU with the header's own
// index functions, in both store forms, and checks that every element of every row is written exactly once, with the value of its
// (byte, bit, column), and nothing else is touched.
//   steps_plan walk C n        both store forms over n input bytes with C columns
//   steps_plan f16             "v bits" for every v in -2047 .. 2047, and the two bit-column values
//   steps_plan pieces n bs run the staged call's piece lengths
//   steps_plan layout L A fmt flags   the layout's fields, or "invalid"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../weath3rb0i_amd/csrc/w3_steps_plan.h"

using namespace w3;

static int fail(const char *what, uint64_t a, uint64_t b) {
    fprintf(stderr, "FAIL %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

static int walk(uint32_t C, uint64_t n, bool staged) {
    const uint64_t elems = steps_rows_bytes(n, C) / 2;
    if (elems != 8 * n * C) return fail("rows bytes", elems, 8 * n * C);
    std::vector<uint64_t> out(elems + 64, 0);          // (64 guard elements behind the rows)
    std::vector<uint32_t> writes(elems + 64, 0);
    std::vector<uint64_t> image((size_t)W3_STEPS_TILE * 8 * C);
    if (steps_lds_bytes(C) != 8192 + image.size() * 2) return fail("lds bytes", steps_lds_bytes(C), image.size() * 2);
    const uint64_t tiles = steps_tiles(n);
    uint64_t covered = 0;
    for (uint64_t t = 0; t < tiles; t++) {
        const uint32_t cnt = steps_tile_bytes(n, t);
        if (cnt == 0 || cnt > W3_STEPS_TILE) return fail("tile bytes", t, cnt);
        covered += cnt;
        std::fill(image.begin(), image.end(), ~0ull);
        for (uint32_t lane = 0; lane < cnt; lane++)
            for (uint32_t k = 0; k < 8; k++)
                for (uint32_t col = 0; col < C; col++) {
                    const uint32_t e = steps_tile_elem(lane, k, col, C);
                    if (e >= image.size() || image[e] != ~0ull) return fail("tile element", e, image.size());
                    image[e] = steps_elem(steps_row(t * W3_STEPS_TILE + lane, k), col, C) + 1;
                }
        const uint64_t base = steps_tile_base(t, C);
        auto store = [&](uint32_t v) -> int {   // one 16-byte vector of the image to the output
            if ((uint64_t)(v + 1) * 8 > image.size()) return fail("image vector", v, image.size());
            for (uint32_t e = 0; e < 8; e++) {
                const uint64_t o = (base + v) * 8 + e;
                if (o >= elems) return fail("store beyond the rows", o, elems);
                out[o] = image[(size_t)v * 8 + e];
                writes[o]++;
            }
            return 0;
        };
        if (staged) {
            const uint32_t nv = steps_tile_vecs(cnt, C);
            for (uint32_t j = 0; j < C; j++)
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint32_t v = j * 64 + lane;
                    if (v < nv && store(v)) return 1;
                }
        } else {
            for (uint32_t lane = 0; lane < cnt; lane++)
                for (uint32_t j = 0; j < C; j++)
                    if (store(steps_lane_vec(lane, j, C))) return 1;
        }
    }
    if (covered != n) return fail("tiles cover", covered, n);
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t k = 0; k < 8; k++)
            for (uint32_t col = 0; col < C; col++) {
                const uint64_t o = (8 * i + k) * C + col;   // the layout of include/w3hip.h, spelled out
                if (writes[o] != 1) return fail("written once", o, writes[o]);
                if (out[o] != o + 1) return fail("value", o, out[o]);
            }
    for (uint64_t o = elems; o < elems + 64; o++)
        if (writes[o]) return fail("guard", o, writes[o]);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "walk")) {
        const uint32_t C = (uint32_t)atoi(argv[2]);
        const uint64_t n = strtoull(argv[3], nullptr, 10);
        if (walk(C, n, true) || walk(C, n, false)) return 1;
        printf("steps plan ok\n");
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "f16")) {
        for (int v = -2047; v <= 2047; v++) printf("%d %u\n", v, (unsigned)steps_f16(v));
        printf("bit %u %u\n", (unsigned)steps_f16_bit(0), (unsigned)steps_f16_bit(1));
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "pieces")) {
        const uint64_t n = strtoull(argv[2], nullptr, 10), bs = strtoull(argv[3], nullptr, 10), run = strtoull(argv[4], nullptr, 10);
        for (uint64_t o0 = 0; o0 < n;) { const uint64_t len = steps_piece_len(n, bs, run, o0); printf("%llu\n", (unsigned long long)len); if (!len) return 1; o0 += len; }
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "layout")) {
        StepsLayout l;
        if (!steps_layout((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 10), (uint32_t)strtoul(argv[5], nullptr, 10), l)) { printf("invalid\n"); return 0; }
        printf("%u %u %u %u %u %u %u %u\n", l.n_cols, l.n_leaves, l.col_mix, l.col_apm0, l.n_apm, l.col_final, l.col_bit, l.elem_bytes);
        return 0;
    }
    fprintf(stderr, "usage: steps_plan walk C n | f16 | pieces n bs run | layout L A fmt flags\n");
    return 2;
}
