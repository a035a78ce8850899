// Host harness for weath3rb0i_amd/csrc/w3_verify.h (tests/test_verify_schedule.py): the sampled verification's schedule — which block
// each sample slot of each call re-predicts — compiled for the CPU and checked against the bound w3hip.h states for W3_OPT_VERIFY.
//   (no arguments)            every block count 1 .. 20,000, with and without a short last block, v in {1, 2, 4, 16, 256}, block sizes
//                             1 KiB / 64 KiB / 4 MiB: in every window of ceil(nb / S) consecutive calls every block is sampled; no index
//                             >= nb; no block twice in one call; the short last block only in the last slot; S x block size within the cap
//   report NB SHORT BS V      blocks never sampled over 8 x nb calls (SHORT = 1: the last block is short)
//   first NB SHORT BS V B     the first call (counted from 0) whose sample holds block B, or -1 (tests/test_gpu_lds_fault.py)
//   series                    series of calls numbered as the library numbers them (w3::VerifyCalls: a count per shape; the pieces of
//                             one w3_encode_blocks call take that call's number): shapes that alternate on one context, and chunked calls
//                             (w3_encode_blocks' pieces), alone and between other shapes — every piece's every block within ceil(nb / S)
//                             of that piece's calls
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#define W3_HD static inline
namespace w3 {
#include "../../weath3rb0i_amd/csrc/w3_verify.h"
}

// the schedule under test (tests/test_verify_schedule.py swaps these two bodies for the pre-round-5 formula)
static uint32_t sample_size(uint32_t nb, bool short_last, uint64_t bs, uint32_t v) {
    (void)short_last;
    return w3::verify_sample_size(nb, bs, v);
}
static uint32_t block_of(uint64_t call, uint32_t s, uint32_t nb, bool short_last, uint32_t S) {
    (void)short_last;
    return w3::verify_block(w3::verify_rotation(call, nb, S), s, nb, S);
}

// how the library numbers calls (w3hip.hip: verify_call, and w3_encode_blocks' pieces; tests/test_verify_schedule.py swaps these two
// bodies for the numbering of rounds 1 - 4: one context-wide count, one number per piece)
static uint64_t number_call(w3::VerifyCalls &vc, uint64_t n, uint64_t bs) {
    return vc.next(n, bs);
}
static uint64_t piece_number(w3::VerifyCalls &vc, uint64_t host_call, uint64_t n_piece, uint64_t bs) {
    (void)vc; (void)n_piece; (void)bs;
    return host_call;
}

static const uint64_t BS[3] = {1024u, 65536u, 4u << 20};
static const uint32_t VS[5] = {1u, 2u, 4u, 16u, 256u};

// one (nb, short_last, S) case: calls [c0, c0 + 2 G); every window of G consecutive calls in there must sample every block
static bool check_case(uint32_t nb, bool short_last, uint32_t S, uint64_t c0, std::vector<uint64_t> &last, std::vector<uint64_t> &stamp, char *why) {
    const uint64_t G = ((uint64_t)nb + S - 1u) / S;
    std::fill(last.begin(), last.begin() + nb, c0);   // last[b]: first call of the current run of calls that have not sampled b
    std::fill(stamp.begin(), stamp.begin() + nb, ~0ull);
    for (uint64_t c = c0; c < c0 + 2u * G; c++) {
        for (uint32_t s = 0; s < S; s++) {
            const uint32_t b = block_of(c, s, nb, short_last, S);
            if (b >= nb) { sprintf(why, "call %llu slot %u: block %u >= nb", (unsigned long long)c, s, b); return false; }
            if (stamp[b] == c) { sprintf(why, "call %llu slot %u: block %u twice in one call", (unsigned long long)c, s, b); return false; }
            stamp[b] = c;
            if (short_last && b == nb - 1u && s != S - 1u) { sprintf(why, "call %llu: the short last block in slot %u of %u", (unsigned long long)c, s, S); return false; }
            if (c - last[b] >= G) { sprintf(why, "block %u: not sampled in calls %llu .. %llu (G = %llu)", b, (unsigned long long)last[b], (unsigned long long)c - 1u, (unsigned long long)G); return false; }
            last[b] = c + 1u;
        }
    }
    for (uint32_t b = 0; b < nb; b++)
        if (c0 + 2u * G - last[b] >= G) {
            sprintf(why, "block %u: not sampled in calls %llu .. %llu (G = %llu)", b, (unsigned long long)last[b], (unsigned long long)(c0 + 2u * G - 1u), (unsigned long long)G);
            return false;
        }
    return true;
}

static int exhaustive() {
    const uint32_t NB_MAX = 20000u;
    const unsigned nth = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::atomic<uint32_t> next{1u};
    std::atomic<unsigned long> cases{0};
    std::atomic<bool> failed{false};
    char fail_msg[512] = "";
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nth; t++)
        th.emplace_back([&]() {
            std::vector<uint64_t> last(NB_MAX), stamp(NB_MAX);
            char why[256];
            for (uint32_t nb; !failed && (nb = next.fetch_add(1u)) <= NB_MAX;) {
                for (int sh = 0; sh < 2; sh++) {
                    const bool short_last = sh == 1;
                    uint32_t done[15], n_done = 0;   // (distinct sample sizes only: the schedule of one (nb, S) is checked once)
                    for (uint64_t bs : BS)
                        for (uint32_t v : VS) {
                            const uint32_t S = sample_size(nb, short_last, bs, v);
                            const uint64_t cap = std::max<uint64_t>((uint64_t)v * (64ull << 20), bs);
                            if (S < 1u || S > nb || (uint64_t)S * bs > cap) {
                                if (!failed.exchange(true)) snprintf(fail_msg, sizeof fail_msg, "nb %u bs %llu v %u: sample size %u outside [1, nb] or over the cap", nb, (unsigned long long)bs, v, S);
                                return;
                            }
                            if (std::find(done, done + n_done, S) != done + n_done) continue;
                            done[n_done++] = S;
                            // calls from one far from 0 (the context's count of calls at that point) and from most multiples of the period
                            if (!check_case(nb, short_last, S, 0x12345677ull * 37u + nb, last, stamp, why)) {
                                if (!failed.exchange(true))
                                    snprintf(fail_msg, sizeof fail_msg, "nb %u%s bs %llu v %u S %u: %s", nb, short_last ? " (short last block)" : "",
                                             (unsigned long long)bs, v, S, why);
                                return;
                            }
                            cases++;
                        }
                }
            }
        });
    for (auto &x : th) x.join();
    if (failed) { printf("FAIL %s\n", fail_msg); return 1; }
    printf("verify schedule ok: %lu cases\n", cases.load());
    return 0;
}

static int report(uint32_t nb, bool short_last, uint64_t bs, uint32_t v) {
    const uint32_t S = sample_size(nb, short_last, bs, v);
    std::vector<char> seen(nb, 0);
    for (uint64_t c = 0; c < 8ull * nb; c++)
        for (uint32_t s = 0; s < S; s++) {
            const uint32_t b = block_of(c, s, nb, short_last, S);
            if (b < nb) seen[b] = 1;
        }
    uint32_t never = 0;
    for (uint32_t b = 0; b < nb; b++) never += !seen[b];
    printf("S %u never sampled %u of %u blocks, short last block %s\n", S, never, nb, short_last ? (seen[nb - 1] ? "sampled" : "never") : "none");
    return 0;
}

static int first(uint32_t nb, bool short_last, uint64_t bs, uint32_t v, uint32_t victim) {
    const uint32_t S = sample_size(nb, short_last, bs, v);
    for (uint64_t c = 0; c < 8ull * nb; c++)
        for (uint32_t s = 0; s < S; s++)
            if (block_of(c, s, nb, short_last, S) == victim) { printf("%llu\n", (unsigned long long)c); return 0; }
    printf("-1\n");
    return 0;
}

// A host call: n bytes in blocks of bs, cut into pieces of at most cb blocks (cb = 0: w3_encode_blocks' default, equal pieces of at most
// 4,096 blocks).  The calls cycle through `kinds` for `rounds` rounds; every piece must have sampled each of its blocks within G_piece
// consecutive calls of its kind.
struct Kind { uint64_t n, bs; uint64_t cb; };
static bool run_series(const std::vector<Kind> &kinds, uint32_t rounds, char *why) {
    struct Piece { uint32_t nb, S, G; bool short_last; uint64_t n; std::vector<uint64_t> last; };
    std::vector<std::vector<Piece>> pcs(kinds.size());
    for (size_t k = 0; k < kinds.size(); k++) {
        const Kind &K = kinds[k];
        const uint64_t nb = (K.n + K.bs - 1) / K.bs;
        uint64_t cb = K.cb;
        if (!cb) { const uint64_t pieces = (nb + 4095) / 4096; cb = (nb + pieces - 1) / pieces; }
        for (uint64_t b0 = 0; b0 < nb; b0 += cb) {
            Piece p;
            p.nb = (uint32_t)std::min(cb, nb - b0);
            p.n = std::min(K.n, (b0 + p.nb) * K.bs) - b0 * K.bs;
            p.short_last = p.n % K.bs != 0;
            p.S = sample_size(p.nb, p.short_last, K.bs, 1);
            p.G = (p.nb + p.S - 1) / p.S;
            p.last.assign(p.nb, 0);
            pcs[k].push_back(p);
        }
    }
    w3::VerifyCalls vc;
    for (uint32_t r = 0; r < rounds; r++)
        for (size_t k = 0; k < kinds.size(); k++) {
            const uint64_t c = number_call(vc, kinds[k].n, kinds[k].bs);
            for (size_t q = 0; q < pcs[k].size(); q++) {
                Piece &p = pcs[k][q];
                const uint64_t cp = piece_number(vc, c, p.n, kinds[k].bs);
                for (uint32_t s = 0; s < p.S; s++) {
                    const uint32_t b = block_of(cp, s, p.nb, p.short_last, p.S);
                    if (b >= p.nb) { sprintf(why, "kind %zu piece %zu: block %u >= %u", k, q, b, p.nb); return false; }
                    if (r - p.last[b] >= p.G) {
                        sprintf(why, "kind %zu (n %llu) piece %zu: block %u not sampled in that kind's calls %llu .. %u (G = %u)", k,
                                (unsigned long long)kinds[k].n, q, b, (unsigned long long)p.last[b], r - 1u, p.G);
                        return false;
                    }
                    p.last[b] = r + 1u;
                }
            }
        }
    for (size_t k = 0; k < kinds.size(); k++)
        for (size_t q = 0; q < pcs[k].size(); q++)
            for (uint32_t b = 0; b < pcs[k][q].nb; b++)
                if (rounds - pcs[k][q].last[b] >= pcs[k][q].G) {
                    sprintf(why, "kind %zu (n %llu) piece %zu: block %u not sampled in that kind's calls %llu .. %u (G = %u)", k,
                            (unsigned long long)kinds[k].n, q, b, (unsigned long long)pcs[k][q].last[b], rounds - 1u, pcs[k][q].G);
                    return false;
                }
    return true;
}

static int series() {
    const uint64_t K64 = 65536, K1 = 1024;
    std::vector<std::vector<Kind>> cases;
    const uint64_t nbs[] = {1, 2, 17, 32, 33, 410, 411, 4096, 4097, 4352, 8192, 15259};
    for (uint64_t a : nbs)                                   // two shapes alternating, whole and ragged
        for (uint64_t b : nbs) {
            if (a == b) continue;
            cases.push_back({{a * K64, K64, 0}, {b * K64 - 1000, K64, 0}});
        }
    cases.push_back({{32 * K1, K1, 0}, {40 * K1 + 5, K1, 0}, {4096 * K1, K1, 0}});   // three shapes
    for (uint64_t nb : {8192ull, 8193ull, 12289ull, 15259ull, 16384ull}) {          // w3_encode_blocks' default pieces
        cases.push_back({{nb * K64, K64, 0}});
        cases.push_back({{nb * K64 - 777, K64, 0}, {32 * K64, K64, 0}});
    }
    cases.push_back({{32 * K1 + 500, K1, 32}});                                         // W3_OPT_HOST_CHUNK_BLOCKS: 32 + a short one
    cases.push_back({{41 * 4096 + 1234, 4096, 7}});                                     // 6 pieces of 7 blocks, the last one short
    cases.push_back({{64 * K1, K1, 32}, {100 * K1, K1, 7}});
    char why[512];
    for (size_t i = 0; i < cases.size(); i++) {
        uint32_t maxG = 1;
        for (const Kind &k : cases[i]) {
            const uint32_t nb = (uint32_t)((k.n + k.bs - 1) / k.bs);
            maxG = std::max(maxG, (nb + 15u) / 16u);
        }
        if (!run_series(cases[i], 3 * maxG + 2, why)) { printf("FAIL series case %zu: %s\n", i, why); return 1; }
    }
    printf("verify series ok: %zu cases\n", cases.size());
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "series")) return series();
    if (argc == 7 && !strcmp(argv[1], "first"))
        return first((uint32_t)atol(argv[2]), atoi(argv[3]) != 0, (uint64_t)atoll(argv[4]), (uint32_t)atol(argv[5]), (uint32_t)atol(argv[6]));
    if (argc == 6 && !strcmp(argv[1], "report"))
        return report((uint32_t)atol(argv[2]), atoi(argv[3]) != 0, (uint64_t)atoll(argv[4]), (uint32_t)atol(argv[5]));
    if (argc != 1) { fprintf(stderr, "usage: %s [report NB SHORT BS V | first NB SHORT BS V B | series]\n", argv[0]); return 2; }
    return exhaustive();
}
