/*
 * w3hip.h — C ABI of the MI355X-native weath3rb0i hot path (libw3hip.so).
 *
 * The reference (mitiko/weath3rb0i) is a CPU-only Rust crate with no FFI or
 * plugin interface; its seams are Rust traits and two private functions in
 * src/main.rs.  This header is the drop-in boundary a Rust shim would bind
 * (see INTEGRATION.md for the `extern "C"` block).  Each entry point cites
 * the reference interface it replaces (paths under /root/reference/src).
 *
 * Conventions: plain pointers and sizes; caller owns every buffer; every call
 * returns 0 (W3_OK) or a negative W3_E_* code — nothing panics or throws
 * across the ABI (the reference aborts on panic, Cargo.toml:24).  A w3_ctx is
 * bound to one GPU and is NOT thread-safe (the reference is single-threaded,
 * Cargo.toml:14-15).  There is no CPU fallback: without a HIP device
 * w3_ctx_create fails with W3_E_HIP.
 */
#ifndef W3HIP_H
#define W3HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W3_ABI_VERSION 8

/* ---- error codes --------------------------------------------------------- */
enum {
    W3_OK            =  0,
    W3_E_INVALID     = -1,  /* bad argument / malformed model spec                    */
    W3_E_NOSPACE     = -2,  /* out_cap too small; *out_len holds the size needed      */
    W3_E_HIP         = -3,  /* HIP runtime error (w3_last_error has the text)         */
    W3_E_UNSUPPORTED = -4,  /* valid spec the device path does not implement          */
    W3_E_NOMEM       = -5,  /* device workspace does not fit                          */
    W3_E_FORMAT      = -6,  /* bad container magic (main.rs:123-124 assert_eq!) or a block length table that
                               claims more compressed bytes than the input buffer holds */
    W3_E_CORRUPT     = -7   /* a decoded block does not match its CRC-32 (the *_checked calls and w3_crc32_verify_device);
                               w3_last_error names the first bad block and the count */
};

/* ---- model spec ----------------------------------------------------------
 * Mirrors the compile-time composition done in init_model() (main.rs:146-152)
 * as a caller-owned, read-only POD: the model tree in POSTFIX order.
 *   leaf  W3_NODE_ORDERN : OrderN::new(bits, align)              models/ordern.rs:14-23
 *                          history = W3_HIST_RAW / W3_HIST_AC / W3_HIST_HUFF makes it
 *                          OrderNEntropy::new(bits, align, hist) models/ordern_entropy.rs:15-24
 *                          (RawHistory history/raw_history.rs; ACHistory::new(max_bits,
 *                          StationaryModel::from_table(table)) history/ac_history.rs:16-19;
 *                          HuffHistory history/huff_history.rs:9-76 with the two code tables
 *                          spec->huff[node.reserved], see w3_huff_table below)
 *                          frozen=1 wraps it in FrozenModel      models/frozen.rs:7-11
 *                          Order0 == (11,3), Order1 == (19,3)    models/order0.rs, order1.rs
 *                          (bijective re-indexing, bin/cmp/main.rs:14-24)
 *   node  W3_NODE_BEST_OF_TWO : BestOfTwoModel::new(a, b)        models/mod.rs:42-75
 *                          pops the two preceding subtrees (a pushed first).
 *
 * BUILD-DEFINED nodes (SURVEY §8 A19 ii-v: the reference ships the primitives but no model
 * that uses them; README.md:6-10 lists "12-bit state table" and "APM mixers" as goals):
 *   leaf  W3_NODE_SLOT_STATE : state-table CM leaf per docs/hashslots.md — context = the
 *                          previous `bits` (= order, 0..7) bytes, hashed once per nibble into a
 *                          HashMap of 2^log_cells Cells (hashmap.rs:1-71); each Slot holds the 15
 *                          12-bit NaiveStateTable states of one nibble (hashmap.rs:73-129,
 *                          state_table/naive.rs); P(1) = StateTable::p(state), update =
 *                          StateTable::next.  Tag miss = the reference's TODO (hashmap.rs:64-68):
 *                          least-observed slot is overwritten.
 *   node  W3_NODE_APM       : adaptive probability map over stretch(p) ("APM mixers"): pops one
 *                          subtree.  align = context kind (W3_APM_ORDER0: partial byte, 256 rows;
 *                          W3_APM_ORDER1: partial byte | previous byte << 8, 65536 rows),
 *                          max_bits = adaptation rate (1..15).  Only as a chain at the root.
 *   node  W3_NODE_MIX       : logistic mixer with learned weights (integer-exact, fresh per block): pops the
 *                          N = bits (2..8) preceding subtrees, each a single leaf (W3_NODE_ORDERN of any history, not frozen, or
 *                          W3_NODE_SLOT_STATE).  align = weight-set selector (W3_MIX_ONE: one set; W3_MIX_ORDER0: 256 sets, row
 *                          c0 = the partial byte with its leading 1, as an ORDER0 APM row; row 0 is unused), max_bits = rate
 *                          (4..20), every other field 0.  State w[S][N] int32, every weight starts at 65536 / N (65536 = 1.0),
 *                          WMAX = 2^20 - 1.  Per step, with the leaves' p_i before the bit in spec leaf order and the row before the bit:
 *                              s_i = stretch[p_i >> 4]                     (-2047 .. 2047)
 *                              dot = sum_i ((w_i * s_i) >> 8)              (int32, arithmetic shifts = floor)
 *                              d   = clamp(dot >> 8, -2047, 2047),  p = squash[d + 2047]        (the node's output)
 *                              err = (bit << 16) - p
 *                              w_i = clamp(w_i + ((s_i * err + (1 << (rate - 1))) >> rate), -WMAX, WMAX)
 *                          The whole step is 32-bit arithmetic (csrc/w3_mix_plan.h is its one copy).  A spec has at most one MIX
 *                          node, its N leaves are all the spec's leaves, and only W3_NODE_APM nodes may follow it.  Bad field
 *                          values or nothing to pop: W3_E_INVALID.  Valid shapes that are not built — a BestOfTwo or frozen leaf
 *                          under it, leaves beside it, a second MIX, MIX after an APM — W3_E_UNSUPPORTED.  Not exported:
 *                          w3_export_steps_* and w3_steps_layout_of return W3_E_UNSUPPORTED for a spec with a MIX node.
 *                          Encode: W3_PATH_TWOPHASE runs the mixer as a stage between the predict kernels and the APM stages
 *                          (k_lmix, csrc/w3_lmix.h; w3_timing.mix_ms), W3_PATH_GENERIC the lane-per-block kernels, W3_PATH_AUTO the
 *                          stage only for shapes at which it has been measured to win, else the lane kernels; the
 *                          streams are the same.  Decode: the sixteen-lane decoder for W3_MIX_ORDER0 where w3_decode_spec_covers
 *                          says so (the 15 nodes of a nibble's tree have 15 different rows), else the lane-per-block kernels.
 *   leaf  W3_NODE_ORDERN with history = W3_HIST_MATCH : the match model, OrderNEntropy(11, 3, MatchHistory(min_len, log_slots))
 *                          (integer-exact, fresh per block; csrc/w3_match_plan.h is the one copy of its arithmetic).
 *                          bits = 11, align = 3, max_bits = min_len m (2..4), log_cells = log_slots L (8..20); table, reserved and
 *                          frozen as for a W3_HIST_RAW leaf.  At byte boundary i of a block x, for k in (m, 2m) and i >= k:
 *                              h_k = ((big-endian integer of x[i-k .. i-1]) * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - L)
 *                              c_k = T_k[h_k], then T_k[h_k] = i              (two tables of 2^L u32, 0 = empty at the block start)
 *                              v_k = bytes of agreement of x[.. i-1] and x[.. c_k-1], at most min(32, c_k); 0 when c_k = 0
 *                          the candidate is (c_2m, v_2m) if v_2m > v_m, else (c_m, v_m); v = 0 predicts nothing; else e = x[c] and
 *                          lq = v for v < 16, 16 + ((v - 16) >> 2) above.  hash() at bit position j (MSB first) is
 *                          (lq << 1) | bit (7-j) of e while the j known bits of the byte equal e's, else 0 (at most 41).
 *                          m or L out of range: W3_E_INVALID.  bits != 11, align != 3 or a second match leaf in one spec:
 *                          W3_E_UNSUPPORTED.  Otherwise an ORDERN leaf like any other (under BestOfTwo, under a MIX, APM stages
 *                          behind, frozen).  Encode: W3_PATH_TWOPHASE computes the keys with one wavefront per block (k_match_keys,
 *                          csrc/w3_match.h; w3_timing.match_ms); decode and W3_PATH_GENERIC: the lane-per-block kernels
 *                          (w3_decode_spec_covers is 0), or — W3_OPT_VARIANT bit 4096 — the sixteen-lane decoder ("which kernels
 *                          decode" below).  w3_export_counters* and w3_export_entropy_* return W3_E_UNSUPPORTED.
 */
enum { W3_NODE_ORDERN = 1, W3_NODE_BEST_OF_TWO = 2, W3_NODE_SLOT_STATE = 3, W3_NODE_APM = 4, W3_NODE_MIX = 5 };
enum { W3_HIST_NONE = 0, W3_HIST_RAW = 1, W3_HIST_AC = 2, W3_HIST_HUFF = 3, W3_HIST_MATCH = 4 };
enum { W3_APM_ORDER0 = 0, W3_APM_ORDER1 = 1 };
enum { W3_MIX_ONE = 0, W3_MIX_ORDER0 = 1 };
#define W3_MIX_MAX_INPUTS 8
#define W3_MAX_NODES  31
#define W3_MAX_LEAVES 16
#define W3_MAX_APM    4
#define W3_MAX_HUFF   4

typedef struct w3_node {
    uint8_t  kind;      /* W3_NODE_*                                  */
    uint8_t  bits;      /* bits_in_context   (1..32)                  */
    uint8_t  align;     /* alignment_bits    (0..7, <= bits)          */
    uint8_t  history;   /* W3_HIST_*                                  */
    uint8_t  max_bits;  /* ACHistory max_bits (0..32); W3_HIST_MATCH: min_len (2..4) */
    uint8_t  frozen;    /* 1 = FrozenModel wrapper                    */
    uint8_t  log_cells; /* SLOT_STATE: HashMap log_cell_count (1..24); W3_HIST_MATCH: log_slots (8..20) */
    uint8_t  reserved;  /* W3_HIST_HUFF: index into spec->huff         */
    uint16_t table[8];  /* StationaryModel table, index 0 = MSB       */
} w3_node;

/* The two code tables of a HuffHistory (history/huff_history.rs:9-15): (code, len) of every byte and of every
 * partial-byte symbol (1 << bit_len | the bit_len bits seen), codes already bit-reversed as HuffHistory::new leaves
 * them (:21-25, :38-42).  Caller-supplied like StationaryModel's table: w3_huff_tables() builds them the way
 * HuffHistory::new does, or pass tables produced by the reference itself. */
typedef struct w3_huff_table {
    uint16_t code[256];     uint8_t len[256];
    uint16_t rem_code[256]; uint8_t rem_len[256];
} w3_huff_table;

/* Zero-initialise the struct before filling it (n_huff and huff are read even when no leaf uses HuffHistory:
 * n_huff > W3_MAX_HUFF, or n_huff != 0 with huff == NULL, is W3_E_INVALID; the tables themselves are only read when a
 * W3_HIST_HUFF leaf refers to them). */
typedef struct w3_model_spec {
    uint32_t n_nodes;
    w3_node  nodes[W3_MAX_NODES];
    uint32_t n_huff;               /* table sets referenced by W3_HIST_HUFF leaves (<= W3_MAX_HUFF) */
    const w3_huff_table *huff;     /* caller-owned, read-only; may be NULL when n_huff == 0          */
} w3_model_spec;

/* ---- lifecycle ------------------------------------------------------------ */
typedef struct w3_ctx w3_ctx;

/* One ctx per process and GPU; owns device workspace + a HIP stream. */
int         w3_ctx_create(int device, w3_ctx **out);
void        w3_ctx_destroy(w3_ctx *ctx);
const char *w3_strerror(int code);
const char *w3_last_error(const w3_ctx *ctx);
int         w3_abi_version(void);

/* 0 if the spec is well-formed AND implemented on the device. */
int         w3_spec_validate(const w3_model_spec *spec);

/* Options */
enum {
    W3_OPT_PATH   = 1,  /* W3_PATH_*: which device implementation encode uses      */
    W3_OPT_TIMING = 2,  /* 1 = record per-kernel hipEvent timings (w3_get_timing) */
    W3_OPT_CODER  = 3,  /* two-phase coder kernel: 0 = k_coder_x4 (default; w3_encode_submit and the half-CU variant run k_coder_x5 in its
                           place), 1 = k_coder_fast, 2 = robust k_coder only, 3 = k_coder_x2, 4 = k_coder_x3, 5 = k_coder_x5 */
    W3_OPT_ACC_LIMIT = 4, /* test hook (19..46): accumulator fill at which the fast coder hands a block back */
    W3_OPT_DEBUG_STAMPS = 5, /* diagnostic: 1 = the partitioned predict kernel sums s_memtime per phase */
    /* 6 was W3_OPT_PARTS (block ranges of ONE call pipelined on streams; measured useless, ABI v5): superseded by
       w3_encode_submit / w3_encode_wait, which pipeline successive CALLS */
    W3_OPT_VARIANT = 7, /* cross-check hook for the tests: bit mask of alternative, bit-exact implementations — 1 = Counter rounds
                           with ballots instead of returning LDS adds, 2 = 4-bit partition passes, 4 = order-2 partition from
                           scratch, 8 = CM decoder without LDS staging, 16 = no side stream, 64 = synchronous calls use the half-CU
                           kernel shapes of the submit / wait pipeline, 128 = submitted calls use the plain shapes, 256 = slot-state
                           leaves always on k_slot (lane per block, hash map in HBM), 512 = always on the sorted replay (wavefront per
                           block, no table; default: the replay below 7,000 blocks, k_slot from there on), 1024 = decode on the
                           lane-per-block kernels only (default: sixteen lanes per block where k_decode_spec applies; AC over Huffman: k_aoh in
                           place of k_aoh_decode_spec), 2048 = AC over Huffman: the full decode w3_aoh_decode_blocks[_device] too runs the
                           sixteen-lane decoder where it covers (the ranges calls do by default), 4096 = a spec with a match-model leaf
                           (W3_HIST_MATCH) decodes on the sixteen-lane decoder too, where the rest of the spec is covered (default: the
                           lane kernels; "which kernels decode" below).  0 = defaults.
                           32 = FAULT INJECTION (test hook of the sampled verification): one LDS-add round of every block returns two
                           lanes each other's value (in the kernels W3_OPT_FAULT_KERNELS names); refused (W3_E_INVALID) unless
                           W3_OPT_VERIFY is on, so it cannot corrupt output */
    W3_OPT_SLOT_BUDGET_MB = 8, /* cap (MiB) on the device memory one batch of slot-state hash maps may take; 0 = derive from free memory */
    W3_OPT_VERIFY = 9,  /* v = 1 (default) .. 256: after every two-phase predict that used returning LDS adds — whose lane-ordered resolution
                           is measured, not documented by the ISA — max(16, nblocks * v / 256) sampled blocks (at most nblocks, at most v x 64 MiB of
                           input; the sample ROTATES from call to call) are predicted again with ballot rounds
                           and compared on the device; on a mismatch the call is re-encoded on the ballot path (w3_timing.n_lds_faults) and the
                           context stays there.  Cost at 1e9 B beside the coder: v = 1 +1.0 ms per 67.5 ms step, v = 2 +1.3, v = 4 +2.1.
                           RESIDUAL RISK, per call: a SYSTEMATIC change of the hardware's behaviour shows in any block and is caught by the
                           first call; a fault confined to ONE block is missed with probability 1 - S / nblocks per call.  COVERAGE BOUND
                           (csrc/w3_verify.h, proved for every block count up to 20,000 and for series of alternating shapes and chunked
                           calls by tests/test_verify_schedule.py): the rotation counts the context's calls PER SHAPE (n, block size) —
                           whichever job slot a call of w3_encode_submit lands on, whatever calls of other shapes lie between them — and
                           every block, the short last one included, is in the sample of at least one of any ceil(nblocks / S) calls of
                           one shape (at one v): just over 256 / v calls for large inputs (259 at 1e9 B in 64 KiB blocks),
                           ceil(nblocks / 16) for small ones (and more where the 64 MiB x v cap binds).  A w3_encode_blocks call counts
                           once, with its own shape, and every piece it is cut into (W3_OPT_HOST_CHUNK_BLOCKS) takes that call's number:
                           each piece's blocks are covered within ceil(piece blocks / S) such calls.  A call re-run after a detected fault
                           or a stripe overflow keeps its number.  NOT covered: a context that cycles through more than 256 shapes (the
                           count of a forgotten shape starts again at the context's count of calls).  A fault that hits each block independently with
                           probability q is missed with probability (1 - q)^S, S = the sample size.  A full in-round check needs a second returning LDS atomic per add (measured
                           +4.1 % of the step for the atomics alone, and no LDS left for its shadow tables) and was not built.  Full coverage = decode the output (w3_decode_blocks_device shares no kernel with the
                           predict phase; bench.py does that for every block of its last step).  A stored CRC table (w3_crc32_blocks_device on the input, beside the
                           encode) makes that check possible without the input: w3_crc32_verify_device on the decoded output.  0 = off */
    W3_OPT_TUNE = 11,   /* scheduling / layout experiments (bit mask; output is identical whatever is set).  Bits 0 – 14: the submit / wait
                           pipeline's arrangements and the slot replay's shapes (HISTORY.md 2.8); 15: rank kernels with eight wavefronts per half
                           CU; 16: host-buffer copies on two streams of their own instead of the context's stream; 17 / 18: k_decode_spec with
                           the round-3 table formats / with the nibble-major ones whatever the batch size (default: by size); 19: the general k_decode_spec
                           where the instance specialised for all-raw-history models would run; 20: w3_export_steps_*: the row kernel's direct store form */
    W3_OPT_FAULT_BLOCK = 10, /* test hook, with W3_OPT_VARIANT bit 32: the one block the injected fault hits (-1 = every block, default) */
    W3_OPT_HOST_CHUNK_BLOCKS = 12, /* w3_encode_blocks: blocks per pipelined piece of a host-buffer call (0 = default: equal pieces of at most
                           4,096 blocks; tests use small values to get ragged pieces).  w3_decode_blocks, w3_decode_ranges, w3_crc32_blocks, their
                           *_checked forms and the w3_aoh_* host-buffer calls: blocks per device call (0 = default: 2 GiB worth) */
    W3_OPT_FAULT_KERNELS = 13, /* test hook, with W3_OPT_VARIANT bit 32: bit mask (1 .. 7) of the kernels whose returning LDS adds the injected
                           fault mis-orders — 1 = k_predict_small's rounds (default), 2 = k_rank_sorted's rounds, 4 = k_partition8's
                           cursor adds (two records of one bin swap their slots in the tile: a permutation, never another index) */
    W3_OPT_AOH_BATCH_BLOCKS = 14, /* test hook in the manner of W3_OPT_HOST_CHUNK_BLOCKS: most blocks per batch of the two-phase form of AC over
                           Huffman, and most jobs per batch of its ranges calls and of the sixteen-lane full decode (0 = default: as many
                           as the device memory budget holds; the output is the same) */
    W3_OPT_EXPORT_EPOCH = 15, /* test hook in the manner of W3_OPT_AOH_BATCH_BLOCKS: bytes per epoch of w3_export_counters_device / _staged
                           (0 = default; the result is the same).  A multiple of 1 KiB, at most 2^28: anything else is W3_E_INVALID */
    W3_OPT_WAVE_GRID = 16 /* test hook in the manner of W3_OPT_AOH_BATCH_BLOCKS: most wavefronts the two wavefront-per-block kernels of the
                           two-phase predict phase (k_match_keys of the match-model leaf, k_predict_wave of the Counter leaves no LDS kernel
                           covers) are launched with, so that a wavefront walks several blocks over its private table (0 = default: one per
                           block up to what the chip and the memory budget hold; the output is the same).  The sampled verification's
                           re-prediction takes the same cap.  Negative: W3_E_INVALID.  What a call ran with: w3_last_wave_grid */
};
enum { W3_PATH_AUTO = 0, W3_PATH_GENERIC = 1, W3_PATH_TWOPHASE = 2,
       W3_PATH_SPEC = 3 /* reported only (w3_timing.path of the AC-over-Huffman decode and ranges calls that took the sixteen-lane decoder;
                           w3_last_decode_path after a w3_decode_blocks* / w3_decode_ranges* call that did); W3_OPT_PATH does not accept it */ };
int         w3_ctx_set_option(w3_ctx *ctx, int opt, int64_t value);

/* Upper bound on the concatenated block streams for n input bytes. */
size_t      w3_max_compressed_size(size_t n, size_t block_size);

/* ---- block encode / decode (host buffers) ---------------------------------
 * Replaces the bit loop of compress()/decompress() (main.rs:99-111, 127-140)
 * run once per block with a fresh model + coder: block b's stream is exactly
 * what the reference writes after its 12-byte header for a file holding only
 * that block.  Streams are byte-aligned (ACWriter::flush, io.rs:91-100) and
 * concatenated in block order; block_lens[ceil(n/block_size)] gets the sizes.
 * *out_len is set even on W3_E_NOSPACE.
 * w3_encode_blocks is PIPELINED inside the call (ABI v8): inputs of more than 4,096 blocks are cut into equal pieces of whole
 * blocks, each a w3_encode_host_submit call (below) — piece k+1's input crosses PCIe while piece k is encoded and piece k-1's
 * streams travel back; the output is byte-identical to the one-piece call's.  `in` / `out` may be pageable or pinned
 * (hipHostMalloc / hipHostRegister) memory; pinned buffers make the copies asynchronous.
 * Size limit of ONE DEVICE call (the *_device, submit / wait, stats, predict and sweep entry points): n < 2^32 - 4096 bytes,
 * W3_E_UNSUPPORTED above (a dispatch counts its work-items in 32 bits and the per-byte kernels use one per input byte).  Blocks are
 * independent: a larger device-resident input is split by the caller at block boundaries.  The HOST-buffer calls w3_encode_blocks
 * and w3_decode_blocks take any length, as the reference streams any length (main.rs:97-109): they go through in pieces of at most
 * 2 GiB of input each; w3_encode_blocks_sharded's limit applies to each device's shard.                                          */
int w3_encode_blocks(w3_ctx *ctx, const w3_model_spec *spec,
                     const uint8_t *in, size_t n, size_t block_size,
                     uint8_t *out, size_t out_cap, size_t *out_len, uint32_t *block_lens);

/* in_len = bytes readable at `in`; a length table whose sum exceeds it is rejected with W3_E_FORMAT before
 * anything is read (the reference reads through ACReader, which cannot run past its file: io.rs:23-26). */
int w3_decode_blocks(w3_ctx *ctx, const w3_model_spec *spec,
                     const uint8_t *in, size_t in_len, const uint32_t *block_lens, size_t nblocks,
                     size_t block_size, uint64_t orig_len, uint8_t *out);

/* ---- same, device-resident (no PCIe in the call) ---------------------------
 * d_* are device pointers on ctx's GPU.  `stream` is a hipStream_t; NULL = the
 * ctx's own stream, an ordinary blocking stream, i.e. ordered against work on
 * the legacy default stream like the default stream itself.  The call only
 * enqueues work and reads back one status word, so it can be timed with events
 * on that stream.
 * d_block_lens[nblocks] u32, d_total[1] u64.                                  */
int w3_encode_blocks_device(w3_ctx *ctx, const w3_model_spec *spec,
                            const uint8_t *d_in, size_t n, size_t block_size,
                            uint8_t *d_out, size_t out_cap,
                            uint32_t *d_block_lens, uint64_t *d_total, void *stream);

int w3_decode_blocks_device(w3_ctx *ctx, const w3_model_spec *spec,
                            const uint8_t *d_in, size_t in_len, const uint32_t *d_block_lens, size_t nblocks,
                            size_t block_size, uint64_t orig_len, uint8_t *d_out, void *stream);

/* ---- random access: byte ranges of the block container -------------------------------------------------------------
 * The reference has no counterpart (one stream per file, main.rs:89-144); build-defined on the block container above.  Blocks are
 * coded independently, so a range needs only the blocks it touches, and each of those only up to the last requested byte in it
 * (the arithmetic decoder does not have to reach the end of a stream).  The arguments describing the container are those of
 * w3_decode_blocks / w3_decode_blocks_device; `ranges` (host memory, both variants) are {offset, len} byte ranges of the original
 * data: overlapping, duplicate, unsorted and zero-length ranges are valid.  The output is the ranges' bytes concatenated in request
 * order; *out_len = the sum of their lengths, set even on W3_E_NOSPACE (out_cap too small: nothing is decoded).
 * W3_E_INVALID: nblocks != ceil(orig_len / block_size) (checked first), a range with offset + len > orig_len (u64 wrap included),
 * or a job in flight.  W3_E_FORMAT: a length table that claims more compressed bytes than in_len.
 *   w3_decode_ranges         host buffers; any orig_len and block count, like w3_decode_blocks.  Only the selected blocks' streams
 *                            cross PCIe (gathered into one host staging buffer, one H2D copy), then one D2H copy of the packed output.
 *                            A selection of more than 2 GiB worth of blocks is decoded in several device calls.
 *   w3_decode_ranges_device  device buffers (d_in, d_block_lens, d_out on ctx's GPU; `stream` as in w3_decode_blocks_device); the
 *                            per-call limit on orig_len of the device calls applies.
 * Retained workspace of the context (grown on demand, released by w3_ctx_destroy): the staging buffer the blocks are decoded into
 * (the sum of the blocks' decoded prefixes), the job table (16 bytes per selected block) and the gather's piece list (24 bytes per
 * 64 KiB of output), plus, for the host variant, a pinned host buffer and a device buffer holding the selected streams and the compact
 * length table, and a device buffer for the packed output.                                                                    */
typedef struct w3_range { uint64_t offset; uint64_t len; } w3_range;
int w3_decode_ranges(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                     size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges,
                     uint8_t *out, size_t out_cap, size_t *out_len);
int w3_decode_ranges_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t in_len, const uint32_t *d_block_lens,
                            size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges /* host */, size_t n_ranges,
                            uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream);

/* ---- which kernels decode ------------------------------------------------------------------------------------------------------
 * w3_decode_blocks*, w3_decode_ranges* and their _checked forms run one of two kernel families: the sixteen-lane decoder, which
 * evaluates a nibble's whole context tree at once (csrc/w3_decode_spec.h: up to 8 leaves — Counter leaves with alignment_bits >= 2,
 * slot-state leaves — under BestOfTwo nodes or a W3_MIX_ORDER0 mixer, and at most 2 APM stages), or the lane-per-block kernels
 * (everything else, a W3_MIX_ONE mixer and — by default — a match-model leaf among it; W3_OPT_VARIANT bit 1024 asks for them by name,
 * bit 4096 opts a spec with a match-model leaf into the sixteen-lane decoder).  The output is the same.
 *   w3_decode_spec_covers   host only, the twin of w3_aoh_decode_spec_covers: 1 where the sixteen-lane decoder takes a decode of this
 *                           spec under default options, 0 where the lane kernels do, the negative W3_E_* code of w3_spec_validate for
 *                           a spec that call refuses.
 *   w3_decode_spec_covers_variant   the same answer under the W3_OPT_VARIANT bits given (no other option enters it but W3_OPT_TUNE bit 14,
 *                           the two-bit groups, which it takes as off).  A spec with ONE live match-model leaf (W3_HIST_MATCH) is the case
 *                           it exists for: by default such a spec decodes on the lane kernels (w3_decode_spec_covers is 0); with bit 4096
 *                           (decode_match_spec) the sixteen-lane decoder carries the leaf — the row of sixteen lanes does match_advance
 *                           at every byte boundary (csrc/w3_match_spec_plan.h), bit-exact with the lane kernels — wherever the rest of
 *                           the spec is covered.  Still refused under the bit: bit 1024, W3_OPT_TUNE bit 14, a W3_MIX_ONE mixer, a
 *                           Counter leaf with alignment_bits < 2, three APM stages.
 *   w3_last_decode_path     W3_PATH_SPEC or W3_PATH_GENERIC: the family the context's most recent call of those named above launched,
 *                           by the decision actually taken (options included); 0 before any decode.  w3_timing is not touched by a
 *                           decode.  (The AC-over-Huffman family reports through w3_timing.path.)                                  */
int w3_decode_spec_covers(const w3_model_spec *spec);
int w3_decode_spec_covers_variant(const w3_model_spec *spec, uint32_t variant);
int w3_last_decode_path(const w3_ctx *ctx);

/* ---- how many wavefronts walked the blocks --------------------------------------------------------------------------------------
 * out[0] / out[1]: the grids (wavefronts, each with a private table in device memory) of the k_match_keys / k_predict_wave launches
 * of the context's most recent two-phase predict phase (an encode, w3_predict_blocks, the exports), by the sizing actually done
 * (W3_OPT_WAVE_GRID included); 0 where that kernel was not launched, the smallest of several k_predict_wave leaves'.  The sampled
 * verification's launches are not reported.  W3_E_INVALID for a null argument.                                                      */
int w3_last_wave_grid(const w3_ctx *ctx, uint32_t out[2]);

/* ---- integrity: CRC-32 per block, and decodes that verify it -----------------------------------------------------------------
 * The reference has no counterpart (one stream per file, no checksum: main.rs:89-144); build-defined on the block container.  An
 * arithmetic decoder cannot notice a damaged stream: it is told how many bytes to produce and produces them.  A table of one CRC-32
 * per ORIGINAL block, made beside the encode and stored with the container (tools/w3cli.cpp: versions 3 and 4), lets a decode tell.
 * The checksum is CRC-32/ISO-HDLC, the one zlib.crc32 computes: reflected polynomial 0xEDB88320, init and xor-out 0xFFFFFFFF,
 * crc("123456789") = 0xCBF43926, crc("") = 0.  Computed on the device (csrc/w3_crc.h: a wavefront per 64 KiB slice of a block, 1 KiB
 * per load instruction, the slices of a larger block folded; blocks may start at any byte address).
 *   w3_crc32_blocks          host buffers, any n: crc[ceil(n / block_size)]; the input goes up in runs of whole blocks
 *                            (W3_OPT_HOST_CHUNK_BLOCKS: blocks per run, as for w3_decode_blocks).
 *   w3_crc32_blocks_device   device buffers; the per-call limit on n of the device calls applies.  A device caller runs it on d_in on
 *                            the stream of its encode: encode needs no entry point of its own.
 *   w3_crc32_verify_device   compares the blocks of d_data with d_crc[ceil(n / block_size)] (device memory): W3_OK, or W3_E_CORRUPT with
 *                            *bad_block = the lowest block that differs and *n_bad = how many do (UINT64_MAX and 0 when none; either
 *                            pointer may be NULL).  The full device decode with a check is w3_decode_blocks_device (or the w3_aoh_ one),
 *                            then this call on its output.
 *   *_checked                the host full decodes and the four ranges calls with a w3_check behind their arguments.  chk->crc is HOST
 *                            memory, one entry per block of the CONTAINER (nblocks), also for the ranges calls.  chk == NULL or
 *                            chk->crc == NULL: W3_E_INVALID.  Every other argument error, W3_E_NOSPACE, W3_E_FORMAT and W3_E_INVALID for a
 *                            job in flight come first and are the unchecked call's, word for word.  On W3_E_CORRUPT the outputs are written as
 *                            the unchecked call writes them and *out_len is set; the caller discards them.  The full decodes verify every
 *                            block of every run before its bytes leave the device.  The ranges calls decode every block a range touches
 *                            WHOLE (a CRC cannot vouch for a prefix) and verify it in the staging buffer before the gather: W3_OK means
 *                            every touched block is intact to its end, not only the requested bytes; a damaged block that no range touches
 *                            is not seen.  A selection that w3_decode_ranges cuts into several device calls may count a bad block twice.
 *                            The verify adds kernels on the call's stream and 16 bytes to a readback the call waits for anyway.
 * Folding the CRC into the pinned w3_encode_host_submit pipeline (host input would cross PCIe once) is not built: DESIGN.md 7. */
typedef struct w3_check {
    const uint32_t *crc;   /* HOST memory, one entry per block of the container (nblocks) */
    uint64_t bad_block;    /* out: lowest block whose decoded bytes do not match, UINT64_MAX if none */
    uint64_t n_bad;        /* out: how many of the verified blocks do not match */
} w3_check;
int w3_crc32_blocks(w3_ctx *ctx, const uint8_t *in, size_t n, size_t block_size, uint32_t *crc);
int w3_crc32_blocks_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, uint32_t *d_crc, void *stream);
int w3_crc32_verify_device(w3_ctx *ctx, const uint8_t *d_data, size_t n, size_t block_size, const uint32_t *d_crc,
                           uint64_t *bad_block, uint64_t *n_bad, void *stream);
int w3_decode_blocks_checked(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                             size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *out, w3_check *chk);
int w3_decode_ranges_checked(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                             size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges,
                             uint8_t *out, size_t out_cap, size_t *out_len, w3_check *chk);
int w3_decode_ranges_device_checked(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t in_len, const uint32_t *d_block_lens,
                                    size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges /* host */, size_t n_ranges,
                                    uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream, w3_check *chk);
/* (the w3_aoh_*_checked twins are declared with their family, below) */

/* ---- the same encode, asynchronous: two to four calls in flight per context --------------------------
 * The reference codes one bit at a time on one thread (main.rs:103-109); here a call is three phases with different
 * bottlenecks (predict: the store path; APM: LDS round trips; coder: one latency chain per lane on 239 of 256 CUs), and a
 * single call runs them one after the other.  w3_encode_submit only ENQUEUES: call k+1's predict phase then executes beside
 * call k's APM and coder kernels (each job has its own workspace; kernel shapes that share a CU's LDS: DESIGN.md 2.8).
 *   w3_encode_submit  arguments as w3_encode_blocks_device (d_total is required); *job receives a handle (0 .. 3).  The
 *                     input must stay valid and the outputs untouched until the job has been waited for.  `stream`: the
 *                     stream d_in was produced on (the job starts after the work enqueued there so far).  W3_E_INVALID when
 *                     w3_encode_max_in_flight(spec, n, block_size) jobs are in flight already.  Specs the predict kernels do not
 *                     cover, and specs whose slot-state leaves walk hash maps in HBM (7,000 blocks and more), run synchronously
 *                     inside the call (still completed by w3_encode_wait).
 *   w3_encode_max_in_flight  how many submitted calls of this size one context keeps in flight: 4 up to 4,096 blocks, 3 up to
 *                     12,288 — there a call's coder is a latency chain on part of an otherwise idle chip (one 64 KiB block:
 *                     17 ms), so the jobs run free, every code stage on a stream of its own, and the calls' coders overlap
 *                     (enwik8 size: 3,893 -> 9,339 MiB/s) — and 2 beyond (the ordered pair of DESIGN.md 2.8:
 *                     step k's coder beside step k+1's rank kernels; a job workspace is ~70 bytes per input byte).  Specs with
 *                     slot-state leaves: 2 (their event records are 32 bytes per input byte and leaf).
 *   w3_encode_wait    blocks until the job is complete; returns what w3_encode_blocks_device would have returned
 *                     (W3_E_NOSPACE included; d_total holds the need).  Jobs may be waited for in any order.
 * Every other entry point returns W3_E_INVALID while a job is in flight.  Output is byte-identical to the synchronous
 * call's.                                                                                                            */
int w3_encode_submit(w3_ctx *ctx, const w3_model_spec *spec,
                     const uint8_t *d_in, size_t n, size_t block_size,
                     uint8_t *d_out, size_t out_cap,
                     uint32_t *d_block_lens, uint64_t *d_total, void *stream, int *job);
int w3_encode_wait(w3_ctx *ctx, int job);
int w3_encode_max_in_flight(const w3_model_spec *spec /* NULL: a Counter-leaf model */, size_t n, size_t block_size);

/* ---- the host-buffer encode, asynchronous: calls in flight (ABI v8) -------------------------------------------
 * compress() of the reference reads a file and writes a file (main.rs:89-113): a host sees PCIe in, encode, PCIe out.  One
 * synchronous call cannot hide its own first copy in, its last coder chain (8 x block_size dependent steps per lane) and its
 * last copy out; a host with several inputs (files of a directory, main.rs:41-50; pieces of a long stream) keeps CALLS in flight:
 *   w3_encode_host_submit   arguments as w3_encode_blocks; enqueues the H2D of `in` on the context's copy-in stream and — as soon
 *                     as a device job slot is free — the encode behind it (w3_encode_submit); returns at once when `in` is pinned
 *                     memory (pageable: when HIP has staged the input).  `in`, `out`, `block_lens` must stay valid and untouched
 *                     until the job has been waited for.  *hjob receives a handle (0 .. 4).  W3_E_INVALID when
 *                     w3_encode_host_max_in_flight(spec, n, block_size) calls are in flight already.
 *   w3_encode_host_max_in_flight  = w3_encode_max_in_flight + 1: the extra call is the one whose input travels while every
 *                     device job slot is busy.
 *   w3_encode_host_wait     blocks until the job's streams and length table are in the caller's buffers; returns what
 *                     w3_encode_blocks would have returned (W3_E_NOSPACE with *out_len = the size needed included).  The jobs are
 *                     encoded in submission order; waiting for a later one first completes the earlier ones on the device (their
 *                     outputs stay on the device until they are waited for themselves).
 * Not to be mixed with w3_encode_submit jobs on the same context.  Every synchronous entry point returns W3_E_INVALID while a
 * host-buffer job is in flight.  Output byte-identical to w3_encode_blocks.                                                  */
int w3_encode_host_submit(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, size_t block_size,
                          uint8_t *out, size_t out_cap, uint32_t *block_lens, int *hjob);
int w3_encode_host_wait(w3_ctx *ctx, int hjob, size_t *out_len);
int w3_encode_host_max_in_flight(const w3_model_spec *spec /* NULL: a Counter-leaf model */, size_t n, size_t block_size);

/* ---- sharding over several GPUs from ONE process (C, C++ or Rust hosts) ---------------------------
 * Blocks are independent (fresh model + coder each), so they shard with no data-path collective: context r codes the
 * contiguous block range w3_shard_range gives it (block b -> rank floor(b * world / nblocks): rank order = stream
 * order) on its own GPU and host thread; the streams land in `out` at the exclusive scan of the ranks' totals, the
 * length table is the concatenation.  Output identical to w3_encode_blocks on one context.  ctxs[] may name the same
 * device more than once (that is how the path is tested on a 1-GPU box).  Multi-PROCESS jobs (one rank per GPU,
 * bench.py) gather over RCCL instead: weath3rb0i_amd/shard.py.                                                       */
int w3_shard_range(size_t nblocks, int world, int rank, size_t *first_block, size_t *end_block);
int w3_encode_blocks_sharded(w3_ctx *const *ctxs, int n_ctx, const w3_model_spec *spec,
                             const uint8_t *in, size_t n, size_t block_size,
                             uint8_t *out, size_t out_cap, size_t *out_len, uint32_t *block_lens);

/* The same with the data RESIDENT ON THE DEVICES and the gather over xGMI — BASELINE.json's "RCCL gather over xGMI to concatenate
 * per-GPU compressed streams" for a host that is not a torch.distributed program (the reference has no counterpart: it is one
 * thread, Cargo.toml:14-15).  d_in[r] (on ctxs[r]'s device) holds shard r: the bytes of the block range w3_shard_range(nblocks,
 * n_ctx, r) of one stream, n[r] of them (a whole number of blocks for every shard but the last).  The shards are encoded
 * concurrently (one host thread per context); then ONE exchange step: an all-gather of the ranks' totals and, at the offsets of
 * their exclusive scan, grouped ncclSend / ncclRecv of the packed streams and length tables straight to the root's d_out /
 * d_block_lens (device pointers on ctxs[root]'s GPU; every peer has its own xGMI link to the root, so the transfers overlap).
 * totals[r] (host) = compressed bytes of shard r; W3_E_NOSPACE when their sum exceeds out_cap.
 * transport: W3_GATHER_AUTO = RCCL when every context has its own device, device copies otherwise; W3_GATHER_RCCL forces the
 * communicator path (one rank is allowed: that is how a 1-GPU box rehearses the RCCL calls); W3_GATHER_PEER_COPY =
 * hipMemcpyPeerAsync from the root's stream.  RCCL is resolved at the first use (dlopen "librccl.so.1"): libw3hip.so itself
 * does not link it, and W3_E_HIP with w3_last_error(ctxs[0]) = "RCCL not available ..." is returned when it is missing.
 * Output identical to w3_encode_blocks_device on one context over the concatenated shards.                               */
enum { W3_GATHER_AUTO = 0, W3_GATHER_RCCL = 1, W3_GATHER_PEER_COPY = 2 };
/* The same as a STREAM of steps (ABI v8) — the throughput form for a one-process host: every context keeps
 * w3_encode_sharded_max_in_flight(...) = min over the shards of w3_encode_max_in_flight calls in flight on its device, and a step's
 * packed streams are gathered when the step is waited for, while the devices are already coding the next steps (at 8 GPUs a 125 MB
 * shard takes 25.7 ms one call at a time and 12.0 ms with four in flight: DESIGN.md section 5).
 *   w3_encode_sharded_submit  d_in / n as above; enqueues every shard's encode (w3_encode_submit on its context, into staging buffers
 *                     of the context) and returns a step handle (0 .. 3).  Inputs must stay valid until the step has been waited
 *                     for.  Shards that w3_encode_submit runs synchronously (a tail below 8 bytes, lane-per-block specs) are coded
 *                     inside this call, one context after the other (such specs are better served by the one-shot call).
 *                     W3_E_INVALID when w3_encode_sharded_max_in_flight steps are in flight already.
 *   w3_encode_sharded_wait    completes step sjob's encodes, then the exchange step (as above: sizes all-gather + grouped ncclSend /
 *                     ncclRecv to ctxs[root]'s d_out / d_block_lens, or device copies) and returns when the streams have landed;
 *                     totals[r] = compressed bytes of shard r.  Steps may be waited for in any order.
 * Output identical to w3_encode_blocks_sharded_device's.                                                                       */
int w3_encode_sharded_submit(w3_ctx *const *ctxs, int n_ctx, const w3_model_spec *spec, const uint8_t *const *d_in, const size_t *n,
                             size_t block_size, int *sjob);
int w3_encode_sharded_wait(w3_ctx *const *ctxs, int n_ctx, int sjob, int root, uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens,
                           uint64_t *totals, int transport);
int w3_encode_sharded_max_in_flight(const w3_model_spec *spec, const size_t *n, int n_ctx, size_t block_size);
/* w3_rccl_library: the library to dlopen INSTEAD of the usual sonames ("librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1");
 * only before the first gather or status call of the process (W3_E_INVALID afterwards).  w3_rccl_status resolves RCCL now and
 * reports: W3_OK, or W3_E_HIP with the loader's message in msg ("RCCL not available: ...").  Neither needs a device.          */
int w3_rccl_library(const char *path);
int w3_rccl_status(char *msg, size_t cap);
int w3_encode_blocks_sharded_device(w3_ctx *const *ctxs, int n_ctx, const w3_model_spec *spec,
                                    const uint8_t *const *d_in, const size_t *n, size_t block_size, int root,
                                    uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens,
                                    uint64_t *totals, int transport);

/* ---- ACStats, the counting sink (helpers.rs:60-90) -------------------------------
 * Every figure the reference publishes is `csize = bits / 8` from this sink (bin/ordern/main.rs:66-80): write_bit counts
 * 1 + the pending parity bits it resolves, flush adds nothing (:87-89).  block_bits[b] = that count for block b coded
 * alone (u32: blocks below 2^28 bytes); csize of a block = block_bits[b] / 8 (:70-73).  Same kernels as the encode,
 * without the pack; nothing is copied out but the counts.                                                          */
int w3_encode_stats(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, size_t block_size, uint32_t *block_bits);
int w3_encode_stats_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, size_t block_size,
                           uint32_t *d_block_bits, void *stream);

/* ---- parameter sweep (bin/ordern/main.rs:9-80) ----------------------------------
 * OrderN::new(bits[c], aligns[c]) for every configuration c, each through the counting sink on every block, ALL IN ONE
 * LAUNCH (lanes = configurations x blocks; batches only when the Counter tables exceed the device memory).
 * block_bits (host memory) = [ncfg][nblocks] bit counts, configuration-major.  The reference runs the configurations one
 * after the other on one thread; the driver around this call (weath3rb0i_amd/sweep.py) prints its lines.            */
int w3_sweep_ordern(w3_ctx *ctx, const uint8_t *in, size_t n, size_t block_size, const uint8_t *bits, const uint8_t *aligns,
                    size_t ncfg, uint32_t *block_bits);
int w3_sweep_ordern_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, const uint8_t *bits, const uint8_t *aligns,
                           size_t ncfg, uint32_t *block_bits);

/* ---- AC over Huffman (bin/ac-over-huffman/main.rs:46-89), the reference's best-ratio driver ------------------------------------
 * compress() of that driver (:69-89): byte histogram -> package_merge(counts, huffman_size) -> canonical(code_lens) (:74-76); then
 * every input byte's code is walked MSB first ((code >> i) & 1 for i = len-1 .. 0, :79-82) and each of those bits takes the usual step
 * p = model.predict(); model.update(bit); ac.encode(bit, p) (:81-84) with model = OrderN::new(ctx_bits, 0) (:71); ac.flush (:87).  The
 * context is the last ctx_bits bits of the HUFFMAN bit string (it runs across symbol boundaries).  The reference only runs this into
 * ACStats (:72, :88), sweeping huffman_size 7..=15 x ctx_bits 8..=30 (:20-32), and has no decoder for it; here it is also a real
 * encode AND decode on the block container.
 *   Code table  w3_huff_code: canonical()'s output AS IS (not bit-reversed: that is w3_huff_table's form); len 0 = symbol absent, else
 *     1..16.  w3_huff_code_table builds it as the driver does, from the histogram of the WHOLE buffer (:74); W3_E_INVALID for the
 *     reference's three panics (no symbols, huffman_size > 32, too small for the alphabet) and for a huffman_size above 16 that yields
 *     a length above 16 (codes are u16, package_merge.rs:87).  Equal counts / lengths are taken in ascending symbol order, as in
 *     w3_huff_tables below; reference-identical tables for tied histograms are the caller's (pass the crate's own canonical()
 *     output: INTEGRATION.md) — hence every entry point takes the TABLE, never huffman_size.  One distinct symbol gives all-zero
 *     lengths, as in the reference (package_merge of one count is [0]): such a file codes zero bits.
 *   Validation (host, before any launch; W3_E_INVALID otherwise): every len <= 16, code < 2^len, and the table equals canonical(len)
 *     up to a permutation among the symbols of equal length (the codes of one length are one contiguous range: the decoder relies on it).
 *   Model  OrderN(ctx_bits, 0), ctx_bits 1..31; history and first context 0; Model::update = adapt, then advance (models/mod.rs:28-31).
 *   Block container as for every other model: block b is coded alone with a fresh model and coder, its stream byte aligned by flush,
 *     streams concatenated, block_lens[] beside them.  The TABLE is global: one per call, as the driver's is one per file.
 *   Counting sink: block_bits[b] as w3_encode_stats defines it; csize = sum / 8 (helpers.rs:70-73).
 *   A byte whose len is 0: stats and sweep mirror the reference for any table (it contributes no bits); the ENCODE entry points return
 *     W3_E_INVALID when the input holds one (checked on the device), because such output could not be decoded.  A container writer
 *     turns the one-symbol table into len 1, code 0 for that symbol before it encodes (tools/w3cli.cpp, Context.aoh_compress).
 *   Limits: block_size x max len < 2^32; n < 2^32 - 4096 per DEVICE call, the host-buffer encode / decode / stats take any length in
 *     pieces of at most 2 GiB.  Other conventions as the neighbours': *out_len set even on W3_E_NOSPACE, W3_E_FORMAT for a length table
 *     that claims more than in_len, W3_E_INVALID while a job is in flight.
 *   W3_OPT_PATH, for w3_aoh_encode_blocks[_device] and w3_aoh_encode_stats[_device]: W3_PATH_GENERIC runs the fused lane-per-block
 *     kernel k_aoh (csrc/w3_aoh.h).  W3_PATH_TWOPHASE runs the two-phase form, for every valid input (never W3_E_UNSUPPORTED):
 *     k_aoh_pack writes every block's Huffman bit string, k_aoh_predict predicts all its steps with a wavefront per block (64
 *     time-ordered steps per round, the Counter table private to the resident wavefront), k_aoh_coder codes a block per lane from the
 *     stored probabilities; workspace = the strings + 2 bytes per coded bit + one table per resident wavefront, a call that exceeds
 *     the device memory budget goes in batches of whole blocks (W3_OPT_AOH_BATCH_BLOCKS caps a batch, for tests).  The output of the
 *     two forms is identical.  W3_PATH_AUTO takes the form its rule names (W3_AOH_AUTO_* in csrc/w3_aoh.h: the fused kernel for
 *     every shape until the two-phase form has been timed); w3_timing.path tells which.  Decode and the sweep IGNORE the option (the full decode and the sweep run k_aoh): the decoder cannot look ahead (a step's
 *     context is known only when the step before it is decoded), and the sweep already has configurations x blocks lanes.
 *     W3_OPT_TIMING: the fused form fills generic_ms / pack_ms / total_ms (predict_ms and coder_ms stay 0); the two-phase form fills
 *     predict_ms (k_aoh_pack + k_aoh_predict), coder_ms, pack_ms, total_ms, predict_bytes and coder_bytes (generic_ms stays 0).
 * w3_aoh_max_compressed_size: upper bound on the concatenated streams (16 output bits per coded bit); 0 = block_size 0 or an INVALID
 * table (needs no device: the way to validate a table).                                                                          */
typedef struct w3_huff_code { uint16_t code[256]; uint8_t len[256]; } w3_huff_code;
int    w3_huff_code_table(const uint8_t *buf, size_t n, uint8_t huffman_size, w3_huff_code *out);   /* host only; from a device histogram: w3_huff_code_from_counts */
size_t w3_aoh_max_compressed_size(size_t n, size_t block_size, const w3_huff_code *code);
int w3_aoh_encode_blocks(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t n, size_t block_size,
                         uint8_t *out, size_t out_cap, size_t *out_len, uint32_t *block_lens);
int w3_aoh_encode_blocks_device(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t n, size_t block_size,
                                uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens, uint64_t *d_total, void *stream);
int w3_aoh_decode_blocks(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len,
                         const uint32_t *block_lens, size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *out);
int w3_aoh_decode_blocks_device(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t in_len,
                                const uint32_t *d_block_lens, size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *d_out,
                                void *stream);
/* Random access on these streams: w3_decode_ranges / w3_decode_ranges_device (above) for this family — the same conventions, word for
 * word: overlapping, duplicate, unsorted and zero-length ranges are valid; the output is the ranges concatenated in request order;
 * *out_len is set even on W3_E_NOSPACE (nothing is decoded then); W3_E_INVALID for nblocks != ceil(orig_len / block_size) (checked
 * first), a range past orig_len (u64 wrap included), an invalid table or ctx_bits, or a job in flight; W3_E_FORMAT for a length table
 * that claims more than in_len.  The host variant sends only the selected blocks' streams over PCIe (one pinned buffer, one H2D copy,
 * one D2H copy) and cuts selections above 2 GiB worth of blocks into several device calls; the workspace is w3_decode_ranges'.
 * The decoder: one decode job per selected block, served by k_aoh_decode_spec (csrc/w3_aoh_spec.h) — SIXTEEN lanes per job: the 15
 * contexts the next four coded bits can reach are loaded in one round trip, the four steps run in registers with the nibble's own
 * updates forwarded, one store per distinct context — where w3_aoh_decode_spec_covers(ctx_bits) is 1: ctx_bits <= 24, a zero-filled
 * direct table of 4 << ctx_bits bytes per job, jobs in batches under the device memory budget.  Otherwise (ctx_bits 25 .. 31), and
 * under W3_OPT_VARIANT bit 1024, the lane-per-job kernel k_aoh, its exact map sized for the longest job.  W3_OPT_VARIANT bit 2048
 * makes the full decode w3_aoh_decode_blocks[_device] take the sixteen-lane decoder too (without it the full decode runs what it
 * always ran).  w3_timing.path after a decode or ranges call of the family: W3_PATH_SPEC when the sixteen-lane decoder ran,
 * W3_PATH_GENERIC otherwise.  Both decoders read a stream the same way: a stream that is not one of ours decodes to the same bytes. */
int w3_aoh_decode_ranges(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len,
                         const uint32_t *block_lens, size_t nblocks, size_t block_size, uint64_t orig_len,
                         const w3_range *ranges, size_t n_ranges, uint8_t *out, size_t out_cap, size_t *out_len);
int w3_aoh_decode_ranges_device(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t in_len,
                                const uint32_t *d_block_lens, size_t nblocks, size_t block_size, uint64_t orig_len,
                                const w3_range *ranges /* host */, size_t n_ranges, uint8_t *d_out, size_t out_cap, size_t *out_len,
                                void *stream);
int w3_aoh_decode_spec_covers(uint8_t ctx_bits);   /* host only: 1 where the sixteen-lane decoder takes the call */
/* The checked forms (w3_check, above: "integrity"): the same calls with the CRC table of the original blocks behind their arguments. */
int w3_aoh_decode_blocks_checked(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len,
                                 const uint32_t *block_lens, size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *out, w3_check *chk);
int w3_aoh_decode_ranges_checked(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len,
                                 const uint32_t *block_lens, size_t nblocks, size_t block_size, uint64_t orig_len,
                                 const w3_range *ranges, size_t n_ranges, uint8_t *out, size_t out_cap, size_t *out_len, w3_check *chk);
int w3_aoh_decode_ranges_device_checked(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t in_len,
                                        const uint32_t *d_block_lens, size_t nblocks, size_t block_size, uint64_t orig_len,
                                        const w3_range *ranges /* host */, size_t n_ranges, uint8_t *d_out, size_t out_cap, size_t *out_len,
                                        void *stream, w3_check *chk);
int w3_aoh_encode_stats(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t n, size_t block_size,
                        uint32_t *block_bits);
int w3_aoh_encode_stats_device(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t n, size_t block_size,
                               uint32_t *d_block_bits, void *stream);
/* The driver's sweep (:20-32) in ONE call: configuration c = (codes[code_idx[c]], ctx_bits[c]); lanes = configurations x blocks,
 * batched only when the Counter tables exceed the device memory.  block_bits (host memory) = [ncfg][nblocks], configuration-major.
 * n_codes <= 64, ncfg <= 4096.  The driver around it (weath3rb0i_amd/sweep.py, --driver ac-huff) prints the reference's lines. */
int w3_sweep_ac_over_huffman(w3_ctx *ctx, const uint8_t *in, size_t n, size_t block_size, const w3_huff_code *codes, size_t n_codes,
                             const uint8_t *code_idx, const uint8_t *ctx_bits, size_t ncfg, uint32_t *block_bits);
int w3_sweep_ac_over_huffman_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, const w3_huff_code *codes,
                                    size_t n_codes, const uint8_t *code_idx, const uint8_t *ctx_bits, size_t ncfg, uint32_t *block_bits);

/* ---- context statistics export (README.md:9: "output stats from contexts for use by external neural nets") --------
 * The Counter table (`stats`, models/ordern.rs:5 / ordern_entropy.rs:6) of a one-leaf adaptive model after it has seen
 * `in` as ONE stream, i.e. the state the reference's model is in when compress() returns: counters[ctx] = n0 | n1 << 16
 * (models/counter.rs:4-6) for ctx in 0 .. 2^bits_in_context.  bits_in_context <= 28, n <= 2^28.                       */
int w3_export_counters(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, uint32_t *counters);

/* ---- the same for whole inputs of any size, on the device (csrc/w3_export.h) ---------------------------------------
 * For ONE adaptive W3_NODE_ORDERN leaf with history == W3_HIST_NONE, not frozen, bits <= 28, the context of a step is a pure function of
 * the input and a Counter depends on the order of its updates only where it halves.  The input goes through in epochs: per epoch every
 * context's visits are counted by bit value (k_exp_count), added to the table where no count can have reached 65535 (k_ctx_apply), and the
 * few contexts in which one did are replayed exactly by a wavefront each (k_exp_replay).  The result equals w3_export_counters bit for
 * bit.  Every other spec is W3_E_UNSUPPORTED (leaves with an entropy history go through w3_export_entropy_device / _staged below or the
 * one-lane call above, w3_last_error says so).
 *   w3_export_counters_device   d_counters = uint32[2^bits] in DEVICE memory, every entry written.  n < 2^32 - 4096 per call, n == 0 gives
 *                               zeros, stream NULL = the context's, the call synchronises its stream before it returns.
 *   w3_export_counters_staged   a host buffer of ANY length and a host result, staged as w3_histogram stages (pieces of 2 GiB;
 *                               W3_OPT_HOST_CHUNK_BLOCKS: nominal 64 KiB blocks per piece); the table stays on the device from piece to
 *                               piece, the history bits and the offset in the stream are carried across the cuts.
 * Both are W3_E_INVALID while a job is in flight.  w3_export_get_profile: what the last of these calls did — the integer fields always,
 * the times under W3_OPT_TIMING (per kernel only up to 4,096 epochs per piece; total_ms: the pieces' kernels from the first to the last,
 * the staged form's copies to and from the device not included). */
typedef struct w3_export_profile {
    uint64_t epochs, replays, halvings;   /* epochs run; (context, epoch) pairs replayed; halvings the replays applied */
    float count_ms, apply_ms, replay_ms, total_ms;
} w3_export_profile;
int w3_export_counters_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, uint32_t *d_counters, void *stream);
int w3_export_counters_staged(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, uint32_t *counters);
int w3_export_get_profile(const w3_ctx *ctx, w3_export_profile *out);

/* ---- ... and for leaves with an entropy history (csrc/w3_export_entropy.h) -------------------------------------------
 * The general single-leaf entry point: ONE adaptive W3_NODE_ORDERN leaf, not frozen, bits <= 28, history any of W3_HIST_NONE, RAW, AC,
 * HUFF.  ACHistory::hash and HuffHistory::hash are pure functions of the input too (the 64 stream bits before a step; the trailing bytes
 * whose code lengths sum to 32), so per epoch a key stage writes the finished context of every step (one uint32 per step: keyed epochs
 * are at most 2^24 bytes whatever W3_OPT_EXPORT_EPOCH says) and count and replay run over the keys.  NONE and RAW run the kernels of the
 * calls above.  Exact for any caller-supplied w3_huff_table, zero-length codes included (an epoch whose bounded walks meet a run of them
 * is redone by the recurrence: huff_fixed_epochs).  Everything else is W3_E_UNSUPPORTED.  The contracts are those of
 * w3_export_counters_device / _staged: every entry written, n < 2^32 - 4096 for the device form, any length staged, n == 0 gives zeros,
 * W3_E_INVALID while a job is in flight, nothing written on a refusal.  The result equals w3_export_counters bit for bit. */
typedef struct w3_export_entropy_profile {
    w3_export_profile base;      /* epochs, replays, halvings, count/apply/replay/total ms: as for the calls above */
    float    key_ms;             /* the key stage (under W3_OPT_TIMING) */
    uint64_t huff_fixed_epochs;  /* epochs whose Huffman keys were redone by the recurrence */
} w3_export_entropy_profile;
int w3_export_entropy_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, uint32_t *d_counters, void *stream);
int w3_export_entropy_staged(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, uint32_t *counters);
int w3_export_entropy_get_profile(const w3_ctx *ctx, w3_export_entropy_profile *out);

/* ---- per-step statistics: what every model said before every coded bit (csrc/w3_steps.h) ---------------------------
 * README.md:9 again: a network that mixes or post-processes a CM's predictions trains on the predictions, not on a final table.  These
 * calls write one ROW per coded bit: row t = 8 i + k belongs to input byte i and bit k (k = 0: the MSB — the order of w3_predict_blocks'
 * p_out), every value the prediction BEFORE that step's update; blocks restart the model, as everywhere.  Columns, 2 bytes each, C per row:
 *   one per leaf            in the spec's postfix leaf order; a FrozenModel leaf has no stream: the constant 32768
 *   mix                     the root before any APM stage (OpinionMixer2 over the leaves; equals the leaf where there is one)
 *   one per APM stage       in chain order
 *   bit                     with W3_STEPS_COL_BIT: the coded bit (0 / 1; 0.0 / 1.0 in F16)
 * The last model column (col_final) is what the coder is given: it equals w3_predict_blocks' output.  Nobody should hard-code the
 * order: w3_steps_layout_of (host only, no device needed) tells it; col_apm0 and col_bit are UINT32_MAX where there is no such column.
 * Formats, all exact:  W3_STEPS_P_U16      Counter::p / the stage's output as is (uint16)
 *                      W3_STEPS_STRETCH_I16  the build's stretch[p >> 4] (w3_stretch_squash), -2047 .. 2047 (int16)
 *                      W3_STEPS_STRETCH_F16  that integer / 256 as IEEE binary16 — exact: |v| < 2^11, and the division is an exponent
 *                                            shift.  (bfloat16 cannot hold these values exactly and is not offered.)
 *   w3_export_steps_device  d_in, d_rows on ctx's GPU; d_rows 16-byte aligned (W3_E_INVALID), rows_cap >= 8 n C 2 bytes (W3_E_NOSPACE), both
 *                           checked before anything is launched.  n == 0 is W3_OK.  Specs and sizes the two-phase predict kernels do not
 *                           cover (n < 8, block_size > 2^24): W3_E_UNSUPPORTED, as w3_predict_blocks.  W3_E_INVALID while a job is in flight.
 *                           n < 2^32 - 4096 per call: the rows of a larger input do not fit one buffer anyway (1e9 bytes x 6 columns =
 *                           96 GB), a caller walks it in runs of whole blocks.  stream NULL = the context's; the call synchronises it.
 *   w3_export_steps_staged  host input of ANY length, host rows: pieces of whole blocks (W3_OPT_HOST_CHUNK_BLOCKS blocks per piece;
 *                           0 = as many as give 2 GiB of rows).
 * The rows come from the same LDS-add rounds as an encode, and carry the same insurance: the sampled re-prediction (W3_OPT_VERIFY) runs
 * on the leaves' streams before any APM stage; on a mismatch the call predicts again with ballot rounds, counts it in
 * w3_timing.n_lds_faults, and the context stays on them.  W3_OPT_TUNE bit 20: the row kernel's direct store form (same rows).
 * w3_export_steps_get_profile: the last call's times (under W3_OPT_TIMING; sums over the staged form's pieces) and byte counts.
 * Not built: Counter confidence counts as columns, AC-over-Huffman streams, a submit / wait form, several GPUs.          */
enum { W3_STEPS_P_U16 = 0, W3_STEPS_STRETCH_I16 = 1, W3_STEPS_STRETCH_F16 = 2 };
enum { W3_STEPS_COL_BIT = 1 };
typedef struct w3_steps_layout {
    uint32_t n_cols, n_leaves, col_mix, col_apm0, n_apm, col_final, col_bit, elem_bytes;
} w3_steps_layout;
typedef struct w3_steps_profile {
    float    predict_ms, apm_ms, rows_ms, total_ms;   /* predict phase; APM stages and their copies; the row kernel; first to last kernel */
    uint64_t bytes_read, bytes_written;               /* the row kernel's */
    uint32_t n_lds_faults, direct_stores;             /* as w3_timing's; 1 = the row kernel ran its direct store form */
} w3_steps_profile;
int w3_steps_layout_of(const w3_model_spec *spec, uint32_t format, uint32_t flags, w3_steps_layout *out);
int w3_export_steps_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, size_t block_size, uint32_t format,
                           uint32_t flags, void *d_rows, size_t rows_cap, void *stream);
int w3_export_steps_staged(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, size_t block_size, uint32_t format,
                           uint32_t flags, void *rows, size_t rows_cap);
int w3_export_steps_get_profile(const w3_ctx *ctx, w3_steps_profile *out);

/* ---- ... and back: code from a caller's probabilities -------------------------------------------------------------------------------
 * The one number the reference's drivers print for a model — the coded size under the real 32-bit coder (main.rs:103-109) — for a
 * stream of probabilities the CALLER supplies, e.g. a trained mixer's output over the rows above: ac.encode(bit, p) with p = d_p[8 i + k]
 * (uint16, 16-byte aligned, the step order above) in place of model.predict().  There is no model: nothing is predicted or verified.
 * The other arguments and the output are w3_encode_blocks_device's (the block container's streams) and w3_encode_stats_device's (the
 * ACStats bit counts).  The coders need p in 1 .. 65535 (a zero would make the coder's interval empty): d_p is checked on the device
 * first, and with a zero in it the call returns W3_E_INVALID — w3_last_error names the first such step and their count — before any
 * coder kernel is launched and with no output touched.  n < 8 or block_size > 2^24: W3_E_UNSUPPORTED (the two-phase coders' limits).
 * There is NO decode counterpart: a decoder needs p for bit t before it knows bit t - 1, and cannot ask an external network per bit.   */
int w3_encode_probs_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, const uint16_t *d_p,
                           uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens, uint64_t *d_total, void *stream);
int w3_encode_stats_probs_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, const uint16_t *d_p,
                                 uint32_t *d_block_bits, void *stream);

/* ---- the reference's whole-file container ----------------------------------
 * compress()/decompress() of main.rs:89-144: b"w30i" + u64 BE length + ONE
 * stream.  One serial chain => one GPU lane; provided for format parity.
 * Inputs above 2^28 bytes are refused with W3_E_UNSUPPORTED (w3_last_error names the block container as the route:
 * a single lane codes 2^28 bytes in about ten minutes; the reference's format has no blocks to code in parallel). */
int w3_compress_stream(w3_ctx *ctx, const w3_model_spec *spec,
                       const uint8_t *in, size_t n, uint8_t *out, size_t out_cap, size_t *out_len);
int w3_decompress_stream(w3_ctx *ctx, const w3_model_spec *spec,
                         const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, size_t *out_len);

/* ---- per-step probabilities (Model::predict for every bit of every block) --
 * models/mod.rs:12-15 evaluated by the device predict phase; p_out[8*n] u16.
 * Lets a test drive the model surface without the coder.                      */
int w3_predict_blocks(w3_ctx *ctx, const w3_model_spec *spec,
                      const uint8_t *in, size_t n, size_t block_size, uint16_t *p_out);

/* ---- StationaryModel::new(buf) (models/ac_hash/stationary.rs:14-34) ---------
 * Host-side table preparation for ACHistory: 8 Counters by bit position walked
 * over `buf`, table[i] = p().  One host thread; the device forms are below.  */
int w3_stationary_table(const uint8_t *buf, size_t n, uint16_t table[8]);

/* ---- HuffHistory::new(buf, huff_size, rem_huff_size) (history/huff_history.rs:17-55) --------
 * Host-side table preparation: byte histogram (helpers.rs:30-36) -> length-limited Huffman code lengths
 * (entropy_coding/package_merge.rs:1-84) -> canonical codes (:87-117), bit-reversed; the same for the 255 partial-byte
 * symbols.  The reference sorts with sort_unstable_by (:9, :92): among EQUAL counts / lengths its order is an
 * implementation detail of Rust's unstable sort; this implementation takes them in ascending symbol order (the order the
 * reference's own tests show for small inputs).  REFERENCE-IDENTICAL TABLES for a histogram with tied counts or lengths
 * therefore come from the crate itself: a Rust host passes HuffHistory's own tables through w3_model_spec.huff (from_tables in
 * INTEGRATION.md); Rust's unstable sort is not re-derived here.  Model construction, not the hot path.
 * Returns W3_E_INVALID for the reference's panics (no symbols, max length > 32 or too small for the alphabet).      */
int w3_huff_tables(const uint8_t *buf, size_t n, uint8_t huff_size, uint8_t rem_huff_size, w3_huff_table *out);

/* ---- table preparation on the device: the byte histogram and StationaryModel::new (csrc/w3_prep.h) ----------------------------
 * The three preparations above walk the WHOLE input on one host thread.  These calls do the walking on the device, so that input which
 * lives there needs no trip to the host, and build the same tables: the results equal w3_stationary_table, w3_huff_code_table and
 * w3_huff_tables bit for bit.
 *   w3_histogram_device         counts[v] (HOST memory, 256 entries) = how many of the n bytes at d_in equal v.
 *   w3_histogram                the same for a host buffer of ANY length: it goes up through the context's staging buffer in pieces of
 *                               2 GiB (W3_OPT_HOST_CHUNK_BLOCKS: nominal 64 KiB blocks per piece), the pieces' counts are added in 64 bits.
 *   w3_stationary_table_device  table[8] (HOST memory) = w3_stationary_table of the n bytes at d_in: k_stat_count counts the one-bits
 *                               per 4 KiB tile and bit position, k_stat_walk follows the eight Counters from tile to tile with a
 *                               wavefront each and reloads only the tiles in which a Counter halves.
 *   w3_stationary_table_staged  the same for a host buffer of any length, staged as w3_histogram stages; the Counters' state stays on the
 *                               device from piece to piece.
 *   w3_huff_code_from_counts, w3_huff_tables_from_counts   host only: what w3_huff_code_table / w3_huff_tables do behind their own
 *                               histogram loop (those two call these), error codes included; W3_E_UNSUPPORTED for a count above 2^32 - 1
 *                               (the reference counts in u32).
 * The four context calls follow the family's rules: the per-call limit n < 2^32 - 4096 for the _device forms, W3_E_INVALID while a job
 * is in flight, n == 0 is valid (all-zero counts; eight fresh Counters, 32768 each), stream NULL = the context's, and the call
 * synchronises its stream before it returns.  The staged copy is not kept for an encode that follows: DESIGN.md 7.
 * w3_table_prep_profile is the measurement hook of tools/table_prep_rate.py: both preparations once, every kernel between HIP events;
 * hist_rep = copies per counter in k_hist256 (1, 2, 4, 8, 16; the calls above use W3_HIST_REP).                                        */
#define W3_STAT_TILE 4096u    /* bytes per tile of the stationary walk */
#define W3_STAT_BATCH 64u     /* tiles per step of the walk */
#define W3_HIST_REP 16u       /* copies of a wavefront's LDS counters */
typedef struct w3_prep_profile {
    float hist_ms, hist_sum_ms, stat_count_ms, stat_walk_ms;   /* k_hist256, k_hist256_sum, k_stat_count, k_stat_walk */
    uint32_t halvings[8];                                      /* per bit position (0 = the MSB) */
    uint16_t table[8];
    uint64_t counts[256];
} w3_prep_profile;
int w3_histogram(w3_ctx *ctx, const uint8_t *in, size_t n, uint64_t counts[256]);
int w3_histogram_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t counts[256] /* host */, void *stream);
int w3_stationary_table_staged(w3_ctx *ctx, const uint8_t *in, size_t n, uint16_t table[8]);
int w3_stationary_table_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, uint16_t table[8] /* host */, void *stream);
int w3_huff_code_from_counts(const uint64_t counts[256], uint8_t huffman_size, w3_huff_code *out);                          /* host only */
int w3_huff_tables_from_counts(const uint64_t counts[256], uint8_t huff_size, uint8_t rem_huff_size, w3_huff_table *out);   /* host only */
int w3_table_prep_profile(w3_ctx *ctx, const uint8_t *d_in, size_t n, uint32_t hist_rep, w3_prep_profile *out);

/* ---- read-only tables of the CM kernels (host-side; for known-answer tests) -----------
 * w3_state_table: NaiveStateTable (state_table/naive.rs:7-115) as 3963 rows of
 * {prob, next[0], next[1]} — the rows of docs/state_table/state_table.csv.
 * w3_stretch_squash: the build-defined logistic pair, stretch[4096] (index p>>4) and
 * squash[4095] (index d+2047).                                                          */
#define W3_STATE_TABLE_SIZE 3963
int w3_state_table(uint16_t *out /* [3963*3] */);
int w3_stretch_squash(int16_t *stretch /* [4096] */, uint16_t *squash /* [4095] */);

/* ---- device self-test ---------------------------------------------------------
 * Exhaustively compares the kernels' division-free Counter::p with the literal
 * u64 formula (models/counter.rs:13-18) for all 2^32 (c0,c1) states, on the GPU. */
int w3_selftest_counter_p(w3_ctx *ctx, uint64_t *mismatches);

/* Diagnostic: per-phase s_memtime sums of the last partitioned predict kernel (W3_OPT_DEBUG_STAMPS=1):
 * [0] digit histograms, [1] first partition pass, [2] remaining passes, [3] rank loop, [7] blocks.       */
int w3_debug_get_stamps(w3_ctx *ctx, uint64_t out[8]);

/* ---- timing of the last encode call (W3_OPT_TIMING=1) ----------------------- */
typedef struct w3_timing {
    float    predict_ms;   /* context + rank + Counter::p kernels            */
    float    coder_ms;     /* lane-per-block arithmetic coder kernel         */
    float    pack_ms;      /* scan + compaction of the block streams         */
    float    generic_ms;   /* fused lane-per-block kernel (generic path)     */
    float    total_ms;
    uint32_t path;         /* W3_PATH_* actually taken                       */
    uint32_t n_coder_launches;
    uint64_t coder_bytes;  /* algorithmic HBM bytes of the coder launches    */
    uint64_t predict_bytes;
    uint32_t n_recoded_blocks; /* blocks the fast coder handed to the robust coder */
    float    apm_ms;       /* APM stage kernels of the two-phase path (k_apm0 / k_apm1, + k_mix / k_partition they need) */
    float    slot_ms;      /* slot-state leaves: table zero-fill + k_slot launches (also inside predict_ms) */
    uint32_t n_slot_launches; /* k_slot launches (block batches sized to the device memory budget) */
    float    achash_ms;    /* ACHistory key kernels (k_achash_lut + k_achash; also inside predict_ms) */
    uint32_t n_parts;      /* pieces the call was cut into: 1 for every device-resident call, >= 1 for w3_encode_blocks (ABI v8: the
                              times and byte counts of this struct are then sums over the pieces) */
    uint32_t n_lds_faults; /* wavefronts of the sampled verification whose streams differed (W3_OPT_VERIFY); > 0: the call was
                              re-encoded with ballot rounds */
    /* launch durations of the predict phase's kernels (they may overlap in time: side stream, or another job's kernels) */
    uint32_t n_wide;       /* wide Counter leaves (H = 16 / 24) of the spec, in leaf order (at most 4 are timed) */
    float    part_ms[4];   /* k_partition8 / k_partition pass of wide leaf w */
    float    rank_ms[4];   /* k_rank_sorted of wide leaf w */
    float    small_ms;     /* k_predict_small launches of the time-ordered Counter leaves (H <= 8, raw history), together */
    float    mix_ms;       /* logistic mixer stage of the two-phase path (k_lmix / k_lmix_one); 0 for specs without a W3_NODE_MIX */
    float    match_ms;     /* key stage of the match-model leaf on the two-phase path (k_match_keys; also inside predict_ms); 0 without one */
} w3_timing;
int w3_get_timing(const w3_ctx *ctx, w3_timing *out);

#ifdef __cplusplus
}
#endif
#endif
