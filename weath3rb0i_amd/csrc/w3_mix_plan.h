// w3_mix_plan.h — the arithmetic of the logistic mixer node (W3_NODE_MIX, include/w3hip.h) in plain C++, usable from host
// and device (no HIP header; tests/test_mix_step.py compiles it with g++): the ONE copy of the step.  k_lmix / k_lmix_one (w3_lmix.h)
// and the lane kernels (w3_cm.h) call it; tests/mixer_ref.py restates it in Python integers.
//
//     s_i = stretch[p_i >> 4]                                   -2047 .. 2047
//     dot = sum_i ((w_i * s_i) >> 8)                            |w_i * s_i| <= WMAX * 2047 < 2^31; |dot| < 8 * 2^23 = 2^26
//     d   = clamp(dot >> 8, -2047, 2047),  p = squash[d + 2047]
//     err = (bit << 16) - p                                     |s_i * err| < 2^27
//     w_i = clamp(w_i + ((s_i * err + (1 << (rate - 1))) >> rate), -WMAX, WMAX)
// Every shift of a signed value is an arithmetic shift (floor); everything fits int32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define W3_MIX_HD __host__ __device__ __forceinline__
#else
#define W3_MIX_HD inline
#endif

namespace w3 {

enum { MIX_ONE = 0, MIX_ORDER0 = 1 };   // (= W3_MIX_* of include/w3hip.h)
enum { MIX_MIN_INPUTS = 2, MIX_MAX_INPUTS = 8, MIX_MIN_RATE = 4, MIX_MAX_RATE = 20 };
#define W3_MIX_WMAX ((1 << 20) - 1)
#define W3_MIX_ONE_F 65536   // the weight 1.0

W3_MIX_HD bool mix_params_ok(uint32_t n, uint32_t select, uint32_t rate) {
    return n >= MIX_MIN_INPUTS && n <= MIX_MAX_INPUTS && select <= MIX_ORDER0 && rate >= MIX_MIN_RATE && rate <= MIX_MAX_RATE;
}
W3_MIX_HD uint32_t mix_sets(uint32_t select) { return select == MIX_ORDER0 ? 256u : 1u; }             // weight sets S (set 0 of 256 is never used)
W3_MIX_HD uint32_t mix_row(uint32_t select, uint32_t c0) { return select == MIX_ORDER0 ? c0 : 0u; }   // c0: the partial byte with its leading 1
W3_MIX_HD int32_t mix_w_init(uint32_t n) { return (int32_t)(W3_MIX_ONE_F / n); }

W3_MIX_HD int32_t mix_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }
// one input's share of the dot product
W3_MIX_HD int32_t mix_term(int32_t w, int32_t s) { return (w * s) >> 8; }
// the index into squash[] - 2047
W3_MIX_HD int32_t mix_d(int32_t dot) { return mix_clamp(dot >> 8, -2047, 2047); }
W3_MIX_HD int32_t mix_err(uint32_t bit, int32_t p) { return (int32_t)(bit << 16) - p; }
W3_MIX_HD int32_t mix_update(int32_t w, int32_t s, int32_t err, uint32_t rate) {
    return mix_clamp(w + ((s * err + (1 << (rate - 1u))) >> rate), -W3_MIX_WMAX, W3_MIX_WMAX);
}

// The step over n inputs held in arrays (W, S: anything indexable that yields int32 values; with n a compile-time constant the loops
// unroll and the arrays stay in registers).
template <class W, class S>
W3_MIX_HD int32_t mix_predict_d(const W &w, const S &s, int n) {
    int32_t dot = 0;
    for (int i = 0; i < n; i++) dot += mix_term(w[i], s[i]);
    return mix_d(dot);
}
template <class W, class S>
W3_MIX_HD void mix_train(W &w, const S &s, int n, uint32_t bit, int32_t p, uint32_t rate) {
    const int32_t err = mix_err(bit, p);
    for (int i = 0; i < n; i++) w[i] = mix_update(w[i], s[i], err, rate);
}

}   // namespace w3
