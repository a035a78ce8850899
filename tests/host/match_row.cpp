// match_row.cpp — the match-model leaf's byte-boundary work as a row of sixteen lanes does it (weath3rb0i_amd/csrc/w3_match_spec_plan.h,
// what k_decode_spec<.., MATCH> calls) on the host: sixteen simulated lanes decode a block byte by byte — the candidate words and table
// reads after the first nibble, the selected lane's store after the second, the byte's store, then the ten lanes' loads of the compare's
// candidate side and of e — against the lane kernels' serial match_advance (w3_match_plan.h) over the same bytes.  The row knows only
// the bytes it has "decoded": the block is copied byte by byte into a heap buffer of EXACTLY the block's size that starts as 0xA5, and
// every byte index a load touches is asserted inside [0, known).  Stand-alone: tests/test_match_row.py builds it with g++, once more
// under -fsanitize=undefined,address, and with mutant headers that must fail.
// usage: match_row
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
    CHECK((uint64_t)first + count <= known, "load of bytes [%u, %u) with %u bytes known", first, first + count, known);
}
#define W3_MATCH_CHECK(first, count, known) check_idx(first, count, known)
#include "../../weath3rb0i_amd/csrc/w3_match_spec_plan.h"

using namespace w3;

static uint64_t n_boundaries = 0, n_predictions = 0, n_cand_just_stored = 0, n_long_wins = 0, n_cap = 0;

// one block: the row against the serial form
static void walk(const uint8_t *src, uint32_t len, uint32_t m, uint32_t L, const char *what) {
    // the serial truth, over the input
    std::vector<uint32_t> Ts((size_t)2 << L, 0u);
    std::vector<MatchState> want(len);
    {
        uint8_t *in = (uint8_t *)malloc(len);
        memcpy(in, src, len);
        MatchState s;
        for (uint32_t i = 0; i < len; i++) {
            want[i] = s;
            if (i + 1u < len) match_advance(s, Ts.data(), m, L, in, i + 1u, i + 1u);
        }
        free(in);
    }
    // the row, over what it has decoded
    uint8_t *out = (uint8_t *)malloc(len);
    memset(out, 0xA5, len);
    std::vector<uint32_t> T((size_t)2 << L, 0u);
    MatchState st;
    MatchRowNear near;
    uint64_t hist = 0;
    for (uint32_t i = 0; i < len; i++) {
        CHECK(st.e == want[i].e && st.lq == want[i].lq, "%s: len %u m %u L %u boundary %u: row (e %u, lq %u), serial (e %u, lq %u)", what, len, m, L, i,
              st.e, st.lq, want[i].e, want[i].lq);
        const uint32_t byte = src[i];
        // first nibble decoded
        hist = (hist << 4) | (byte >> 4);
        uint32_t cand[MATCH_ROW_LANES][2];
        const bool more = i + 1u < len;
        for (uint32_t r = 0; r < (uint32_t)MATCH_ROW_LANES; r++)
            for (uint32_t t = 0; t < 2u; t++)
                cand[r][t] = more && match_row_active(i + 1u, m, t) ? T[((size_t)t << L) + match_hash(match_row_word(hist, r), m << t, L)] : 0u;
        // second nibble decoded
        hist = (hist << 4) | (byte & 15u);
        if (!more) { out[i] = (uint8_t)byte; break; }
        uint32_t c[2] = {0u, 0u}, writers = 0;
        for (uint32_t r = 0; r < (uint32_t)MATCH_ROW_LANES; r++) {
            if (!match_row_is_writer(r, byte)) continue;
            writers++;
            c[0] = cand[r][0]; c[1] = cand[r][1];
        }
        CHECK(writers == 1u, "%s: %u lanes selected", what, writers);
        for (uint32_t r = 0; r < (uint32_t)MATCH_ROW_LANES; r++)
            if (match_row_is_writer(r, byte))
                for (uint32_t t = 0; t < 2u; t++)
                    if (match_row_active(i + 1u, m, t)) T[((size_t)t << L) + match_hash(match_row_word(hist >> 4, r), m << t, L)] = i + 1u;
        out[i] = (uint8_t)byte;   // lane 0's store, landed before the loads below
        const uint32_t known = i + 1u;
        match_row_push(near, hist);
        uint32_t mine[MATCH_ROW_LANES];
        for (uint32_t r = 0; r < (uint32_t)MATCH_ROW_LANES; r++)
            mine[r] = match_row_lane_load([&](uint32_t p) -> uint32_t { return out[p]; }, near, known, c[0], c[1], r);
        uint32_t v[2], e[2];
        for (uint32_t t = 0; t < 2u; t++) {
            v[t] = match_row_length(&mine[4u * t], c[t]);
            e[t] = mine[8u + t];
        }
        match_row_finish(st, v[0], v[1], e[0], e[1]);
        n_boundaries++;
        n_predictions += st.lq != 0u;
        n_cand_just_stored += (c[0] == i && v[0]) || (c[1] == i && v[1]);
        n_long_wins += match_takes_long(v[0], v[1]);
        n_cap += v[0] == (uint32_t)MATCH_CAP || v[1] == (uint32_t)MATCH_CAP;
    }
    CHECK(memcmp(T.data(), Ts.data(), T.size() * 4u) == 0, "%s: len %u m %u L %u: the tables differ at the end", what, len, m, L);
    free(out);
}

// CRC-32 (reflected 0xEDB88320) of an input: printed for every directed input, so that tests/test_match_row.py can hold it against
// zlib.crc32 of tests/match_ref.py's DIRECTED entry of that name — the inputs rebuilt below are those bytes, not look-alikes
static void print_input(const char *name, const std::vector<uint8_t> &x) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint8_t b : x) { c ^= b; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); }
    printf("input %s %u %08x\n", name, (unsigned)x.size(), c ^ 0xFFFFFFFFu);
}

static uint32_t lcg_state;
static uint32_t lcg(uint32_t mod) { lcg_state = (lcg_state * 1103515245u + 12345u) & 0x7FFFFFFFu; return (lcg_state >> 16) % mod; }

int main() {
    static const uint32_t cfg[4][2] = {{2, 8}, {3, 12}, {4, 16}, {4, 20}};
    // every size 1..40 of several shapes
    for (uint32_t n = 1; n <= 40u; n++) {
        for (uint32_t shape = 0; shape < 6u; shape++) {
            std::vector<uint8_t> x(n);
            lcg_state = 17u * n + shape;
            for (uint32_t i = 0; i < n; i++)
                x[i] = shape == 0 ? 0u : shape == 1 ? 0xFFu : shape == 2 ? (uint8_t)("\x03\x01\x04\x01\x05\x09\x02"[i % 7u]) : shape == 3 ? (uint8_t)lcg(2) : shape == 4 ? (uint8_t)lcg(16) : (uint8_t)lcg(256);
            for (uint32_t k = 0; k < 4u; k++) walk(x.data(), n, cfg[k][0], cfg[k][1], "small");
        }
    }
    // the directed inputs (tests/match_ref.py: DIRECTED), rebuilt here byte for byte (its _lcg is lcg() above; print_input: the proof)
    {
        std::vector<uint8_t> x;
        x.assign(4096, 0); print_input("zeros", x); for (uint32_t k = 0; k < 4u; k++) walk(x.data(), 4096, cfg[k][0], cfg[k][1], "zeros");
        x.assign(70, 0xFF); print_input("ones_short", x); for (uint32_t k = 0; k < 3u; k++) walk(x.data(), 70, cfg[k][0], cfg[k][1], "ones_short");
        x.resize(1024); for (uint32_t i = 0; i < 1024u; i++) x[i] = (uint8_t)(i & 63u);
        print_input("period_64", x);
        for (uint32_t k = 0; k < 3u; k++) walk(x.data(), 1024, cfg[k][0], cfg[k][1], "period_64");
        x.resize(700); for (uint32_t i = 0; i < 700u; i++) x[i] = (uint8_t)("\x03\x01\x04\x01\x05\x09\x02"[i % 7u]);
        print_input("period_7", x);
        for (uint32_t k = 0; k < 3u; k++) walk(x.data(), 700, cfg[k][0], cfg[k][1], "period_7");
        x.clear();
        for (uint32_t j = 0; j < 8u; j++) {   // eight contexts, each followed by 0x55 and then by 0x55 with bit j flipped
            for (uint32_t rep = 0; rep < 2u; rep++) {
                for (uint32_t t = 0; t < 8u; t++) x.push_back((uint8_t)(8u * j + t + 1u));
                x.push_back(rep ? (uint8_t)(0x55u ^ (0x80u >> j)) : (uint8_t)0x55u);
            }
        }
        print_input("mismatch_bits", x);
        for (uint32_t k = 0; k < 3u; k++) walk(x.data(), (uint32_t)x.size(), cfg[k][0], cfg[k][1], "mismatch_bits");
        static const uint32_t mods[3] = {16, 256, 2}, seeds[3] = {5, 11, 3};
        static const char *names[3] = {"nibbles", "bytes", "pairs"};
        for (uint32_t s = 0; s < 3u; s++) {
            x.resize(4096); lcg_state = seeds[s];
            for (uint32_t i = 0; i < 4096u; i++) x[i] = (uint8_t)lcg(mods[s]);
            print_input(names[s], x);
            for (uint32_t k = 0; k < 4u; k++) walk(x.data(), 4096, cfg[k][0], cfg[k][1], names[s]);
        }
        static const char *words[6] = {"the quick brown fox ", "jumps over ", "a lazy dog; ", "quick brown cat ", "over a lazy fox, ", "brown dog jumps "};
        x.clear(); lcg_state = 99u;
        for (uint32_t w = 0; w < 300u; w++) { const char *p = words[lcg(6)]; x.insert(x.end(), p, p + strlen(p)); }
        x.resize(4096);
        print_input("phrases", x);
        for (uint32_t k = 0; k < 3u; k++) walk(x.data(), 4096, cfg[k][0], cfg[k][1], "phrases");
    }
    CHECK(n_predictions > 1000 && n_cand_just_stored > 1000 && n_long_wins > 10 && n_cap > 1000, "the walk missed a state: %llu predictions, %llu candidates just stored, %llu long wins, %llu at the cap",
          (unsigned long long)n_predictions, (unsigned long long)n_cand_just_stored, (unsigned long long)n_long_wins, (unsigned long long)n_cap);
    if (fails) { fprintf(stderr, "FAIL: %d checks\n", fails); return 1; }
    printf("match row ok: %llu boundaries, %llu predictions, %llu with the candidate just stored, %llu long wins, %llu loads checked\n", (unsigned long long)n_boundaries,
           (unsigned long long)n_predictions, (unsigned long long)n_cand_just_stored, (unsigned long long)n_long_wins, (unsigned long long)n_loads);
    return 0;
}
