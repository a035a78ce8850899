// w3_spec.h — host-side parsed form of w3_model_spec: the leaves in in-order (a BestOfTwo tree of any
// shape returns the leftmost leaf of maximal |p - 1/2|; under a W3_NODE_MIX the leaves are the mixer's inputs, in spec order) followed by
// the APM chain applied at the root.
#pragma once
#include "../../include/w3hip.h"

struct ParsedSpec {
    int n_leaves = 0;
    w3_node leaf[W3_MAX_LEAVES];
    int n_apm = 0;
    w3_node apm[W3_MAX_APM];
    bool has_slot = false;
    bool has_mix = false;                 // the leaves feed a logistic mixer (W3_NODE_MIX: bits = inputs, align = selector, max_bits = rate)
    w3_node mix{};
    bool has_match = false;               // one leaf is the match model (W3_HIST_MATCH: max_bits = min_len, log_cells = log_slots)
    uint32_t n_huff = 0;                  // HuffHistory table sets (caller's memory, valid during the call)
    const w3_huff_table *huff = nullptr;
    bool is_cm() const { return has_slot || n_apm > 0 || has_mix; }
};
