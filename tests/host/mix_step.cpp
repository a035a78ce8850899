// mix_step.cpp — the logistic mixer's step (weath3rb0i_amd/csrc/w3_mix_plan.h) against a 64-bit restatement with explicit floor
// divisions, on seeded random and extreme (w, s, p, bit, rate) tuples, every clamp included.  Stand-alone: tests/test_mix_step.py builds
// it with g++, once more under -fsanitize=undefined (the header's arithmetic must stay inside int32), and with mutant headers that must fail.
// usage: mix_step [thousands of random tuples]
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../weath3rb0i_amd/csrc/w3_mix_plan.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 10) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static int64_t floordiv(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
static int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }
static const int64_t WMAX = (1 << 20) - 1;

static int64_t ref_d(const int32_t *w, const int32_t *s, int n) {
    int64_t dot = 0;
    for (int i = 0; i < n; i++) {
        const int64_t prod = (int64_t)w[i] * s[i];
        CHECK(prod >= INT32_MIN && prod <= INT32_MAX, "w * s leaves int32");
        dot += floordiv(prod, 256);
    }
    CHECK(dot > -(1ll << 26) && dot < (1ll << 26), "dot leaves 2^26");
    return clamp64(floordiv(dot, 256), -2047, 2047);
}
static int64_t ref_update(int64_t w, int64_t s, int64_t bit, int64_t p, int64_t rate) {
    const int64_t err = bit * 65536 - p, v = s * err + (1ll << (rate - 1));
    CHECK(v >= INT32_MIN && v <= INT32_MAX, "s * err + round leaves int32");
    return clamp64(w + floordiv(v, 1ll << rate), -WMAX, WMAX);
}

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 16); }
static int32_t rnd_in(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }

static void one_update(int32_t w, int32_t s, uint32_t bit, int32_t p, uint32_t rate) {
    const int32_t got = w3::mix_update(w, s, w3::mix_err(bit, p), rate);
    const int64_t want = ref_update(w, s, bit, p, rate);
    CHECK(got == want, "update(w %d, s %d, bit %u, p %d, rate %u) = %d, want %lld", w, s, bit, p, rate, got, (long long)want);
}
static void one_predict(const int32_t *w, const int32_t *s, int n) {
    const int32_t got = w3::mix_predict_d(w, s, n);
    const int64_t want = ref_d(w, s, n);
    CHECK(got == want, "predict over %d inputs (w0 %d, s0 %d) = %d, want %lld", n, w[0], s[0], got, (long long)want);
    CHECK(got >= -2047 && got <= 2047, "d outside the squash table");
}

int main(int argc, char **argv) {
    const int thousands = argc > 1 ? atoi(argv[1]) : 200;
    // the parameters' ranges and the initial weights
    for (uint32_t n = 0; n < 12; n++)
        for (uint32_t sel = 0; sel < 4; sel++)
            for (uint32_t rate = 0; rate < 24; rate++)
                CHECK(w3::mix_params_ok(n, sel, rate) == (n >= 2 && n <= 8 && sel <= 1 && rate >= 4 && rate <= 20), "mix_params_ok(%u, %u, %u)", n, sel, rate);
    for (uint32_t n = 2; n <= 8; n++) CHECK(w3::mix_w_init(n) == (int32_t)(65536 / n), "mix_w_init(%u)", n);
    CHECK(w3::mix_sets(w3::MIX_ONE) == 1 && w3::mix_sets(w3::MIX_ORDER0) == 256, "mix_sets");
    for (uint32_t c0 = 1; c0 < 256; c0++) CHECK(w3::mix_row(w3::MIX_ORDER0, c0) == c0 && w3::mix_row(w3::MIX_ONE, c0) == 0, "mix_row(%u)", c0);

    // extreme tuples: every combination of the corner values, every rate
    const int32_t ws[] = {-(int32_t)WMAX, -(int32_t)WMAX + 1, -65536, -257, -256, -255, -1, 0, 1, 255, 256, 257, 8192, 21845, 32768, 65536, (int32_t)WMAX - 1, (int32_t)WMAX};
    const int32_t ss[] = {-2047, -2046, -1024, -3, -2, -1, 0, 1, 2, 3, 1024, 2046, 2047};
    const int32_t ps[] = {22, 23, 4096, 32767, 32768, 32769, 61440, 65513, 65514};
    for (int32_t w : ws)
        for (int32_t s : ss)
            for (int32_t p : ps)
                for (uint32_t bit = 0; bit < 2; bit++)
                    for (uint32_t rate = 4; rate <= 20; rate++) one_update(w, s, bit, p, rate);
    for (int n = 2; n <= 8; n++)
        for (int32_t w : ws)
            for (int32_t s : ss) {
                int32_t wa[8], sa[8];
                for (int i = 0; i < 8; i++) { wa[i] = w; sa[i] = s; }
                one_predict(wa, sa, n);                    // all inputs alike: the sum's extremes, d at both clamps
                for (int i = 0; i < 8; i += 2) sa[i] = -s; // alternating signs: floors of negative and positive terms side by side
                one_predict(wa, sa, n);
            }
    // the clamps are reached, not only approached
    { int32_t wa[8], sa[8]; for (int i = 0; i < 8; i++) { wa[i] = (int32_t)WMAX; sa[i] = 2047; }
      CHECK(w3::mix_predict_d(wa, sa, 2) == 2047, "d at the upper clamp"); for (int i = 0; i < 8; i++) sa[i] = -2047; CHECK(w3::mix_predict_d(wa, sa, 8) == -2047, "d at the lower clamp"); }
    CHECK(w3::mix_update((int32_t)WMAX - 5, 2047, w3::mix_err(1, 22), 4) == WMAX, "w at +WMAX");
    CHECK(w3::mix_update(-(int32_t)WMAX + 5, 2047, w3::mix_err(0, 65514), 4) == -WMAX, "w at -WMAX");

    // seeded random tuples and whole steps through the array forms
    for (int it = 0; it < thousands * 1000; it++) {
        const int n = rnd_in(2, 8);
        const uint32_t rate = (uint32_t)rnd_in(4, 20), bit = rnd() & 1u;
        int32_t w[8], s[8], w2[8];
        const bool wide = (rnd() & 3u) == 0;
        for (int i = 0; i < n; i++) {
            w[i] = wide ? rnd_in(-(int32_t)WMAX, (int32_t)WMAX) : rnd_in(-70000, 140000);
            s[i] = (rnd() & 7u) == 0 ? ((rnd() & 1u) ? 2047 : -2047) : rnd_in(-2047, 2047);
            w2[i] = w[i];
        }
        one_predict(w, s, n);
        const int32_t p = rnd_in(22, 65514);
        w3::mix_train(w2, s, n, bit, p, rate);
        for (int i = 0; i < n; i++) {
            const int64_t want = ref_update(w[i], s[i], bit, p, rate);
            CHECK(w2[i] == want, "train: input %d of %d (w %d, s %d, bit %u, p %d, rate %u) = %d, want %lld", i, n, w[i], s[i], bit, p, rate, w2[i], (long long)want);
        }
    }
    if (fails) { fprintf(stderr, "FAIL: %d checks\n", fails); return 1; }
    printf("mix step ok\n");
    return 0;
}
