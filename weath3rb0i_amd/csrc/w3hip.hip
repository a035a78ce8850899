// w3hip.hip — host side of the C ABI declared in include/w3hip.h, plus the
// kernel launches.  MI355X (gfx950) only.  No CPU fallback anywhere in this
// file: without a device every entry point fails with W3_E_HIP.
#include "../../include/w3hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "w3_spec.h"
#include "w3_huff.h"
#include "w3_generic.h"
#include "w3_cm.h"
#include "w3_decode_spec.h"
#include "w3_pack.h"
#include "w3_tables_plan.h"
#include "w3_jobs.h"
#include "w3_twophase.h"
#include "w3_selftest.h"
#include "w3_sweep.h"
#include "w3_aoh.h"
#include "w3_aoh_spec.h"
#include "w3_rccl.h"
#include "w3_crc.h"
#include "w3_prep.h"
#include "w3_export.h"
#include "w3_export_entropy.h"
#include "w3_steps.h"

using namespace w3;

static_assert(sizeof(w3_node) == 24 && sizeof(w3_huff_table) == 1536 && sizeof(w3_model_spec) == 760, "ABI struct layout (tests/test_host_abi.py)");

// ---------------------------------------------------------------------------
// ctx
// ---------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

// A submitted call, kept for the rare redo (stripe overflow, fast-coder hand-back, LDS-order fault, output beyond the realistic bound).
// The spec and its HuffHistory tables are the caller's memory: both are copied, and the copies point at each other.
struct KeptCall {
    w3_model_spec spec{};
    ParsedSpec ps;
    w3_huff_table huff_copy[W3_MAX_HUFF];
    const uint8_t *d_in = nullptr; size_t n = 0, block_size = 0;
    uint64_t vcall = 0;            // the call's number for the verification's rotation (a redo keeps it; w3_encode_blocks: the same for all its pieces)
    void keep(const w3_model_spec *s, const ParsedSpec &p, const uint8_t *d_in_, size_t n_, size_t block_size_) {
        spec = *s; ps = p; d_in = d_in_; n = n_; block_size = block_size_;
        if (p.n_huff) { memcpy(huff_copy, p.huff, sizeof(w3_huff_table) * p.n_huff); spec.huff = ps.huff = huff_copy; }
    }
    KeptCall() = default;
    KeptCall(const KeptCall &) = delete;   // (it points into itself)
    KeptCall &operator=(const KeptCall &) = delete;
};

// One encode in flight: its own workspace, so that call k+1's predict phase can run beside call k's APM and coder kernels
// (w3_encode_submit / w3_encode_wait).  Every synchronous call uses jobs[0]'s.
struct Job {
    int index = 0;                 // its place in w3_ctx::jobs
    TwoPhaseWs tp; DevBuf stripes, flag, bits, offs, huff; hipEvent_t ev[W3_NEV]{};   // the workspace (ev: W3_OPT_TIMING)
    int state = 0;                 // 0 idle, 1 enqueued (w3_encode_wait completes it), 2 ran synchronously inside w3_encode_submit
    hipEvent_t ev_done = nullptr, ev_in = nullptr;
    hipEvent_t ev_a = nullptr, ev_apm = nullptr;   // first predict half through / APM stages through (what the other job's kernels wait for)
    bool code_pending = false;     // the APM + coder + pack stage is not enqueued yet (it goes behind the NEXT job's first predict half)
    uint32_t nb = 0, cap = 0;
    uint32_t *h_status = nullptr;  // pinned: [0, ST_WORDS) the call's status words (w3_jobs.h), then the total compressed bytes
    KeptCall call;                 // for the rare synchronous redo in w3_encode_wait
    uint8_t *d_out = nullptr; size_t out_cap = 0; uint32_t *d_block_lens = nullptr; uint64_t *d_total = nullptr;
    w3_timing tm{};
    w3_timing tm_ev{}; bool tm_snap = false;   // the event times, collected early (a synchronous fallback is about to reuse job 0's events)
    int sync_rc = W3_OK;           // state 2: what the synchronous run inside w3_encode_submit returned
    uint64_t total_out = 0; bool total_valid = false;   // the compressed size w3_encode_wait read from the job's pinned status words
    bool timed = false;
    hipStream_t sc = nullptr;      // the stream this job's code stage runs on (free-running jobs: one each; ordered jobs share s_code[0])
};

// One host-buffer encode in flight (w3_encode_host_submit / w3_encode_host_wait): its own device input / output buffers, so that call
// k+1's input can travel over PCIe while call k is being encoded and call k-1's streams travel back.  One more than the device jobs:
// the extra one is the call whose input is on its way while every device job slot is busy.
#define W3_MAX_HOST_JOBS (W3_MAX_JOBS + 1)
struct HostJob {
    int state = 0;                 // 0 idle, 1 input enqueued (H2D), encode not submitted yet (no device job slot free), 2 encode submitted (djob),
                                   // 3 through on the device (rc / total known), output not fetched yet
    int djob = -1, rc = W3_OK;
    uint64_t seq = 0, total = 0;
    DevBuf d_in, d_out, d_lens, d_total;
    hipEvent_t ev_d2h = nullptr;
    KeptCall call;
    size_t nb = 0, dcap = 0;
    uint8_t *out = nullptr; size_t out_cap = 0; uint32_t *block_lens = nullptr;
    w3_timing tm{};
};

struct w3_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int opt_path = W3_PATH_AUTO;
    int opt_timing = 0;
    w3_timing timing{};
    int last_decode_path = 0;   // w3_last_decode_path: the kernel family of the most recent w3_decode_* call (lane_run), 0 before any
    uint32_t last_wave_grid[2] = {0u, 0u};   // w3_last_wave_grid: the {k_match_keys, k_predict_wave} grids of the most recent predict phase (twophase_predict_a)
    // workspace that is not a job's
    DevBuf tables, lens, total, io_in, io_out, coffs, misc, cm_luts, achash_luts, sweep;
    DevBuf aoh;   // AC over Huffman (w3_aoh.h): code tables in device form, configurations, block bit lengths, maxima and flags
    // the random-access decode (w3_decode_ranges*): the staging buffer the jobs decode into, the job table + gather pieces (+ for the
    // host variant the compact length table and the selected streams behind them), and the host variant's pinned host copy of those
    DevBuf rg_stage, rg_meta;
    void *h_rg = nullptr; size_t h_rg_cap = 0;
    // CRC-32 per block (w3_crc.h): [0, 16) the verify's result {lowest mismatching segment, mismatches}, from byte 256 on the slices' CRCs;
    // crc_tab: a table on its way to or from a host caller; crc_res: where the result lands on the host
    DevBuf crc_ws, crc_tab;
    DevBuf prep_ws;   // table preparation (w3_prep.h): the counts, the walk's state, the histogram's partials, the tiles' counts (W3_PREP_WS_*)
    // the parallel statistics export (w3_export.h): the delta table D (all zero between calls: exp_d_zero = the bytes known to be), the
    // staged form's table, the replay list, the kernels' stats words
    DevBuf exp_d, exp_s, exp_list, exp_stats;
    size_t exp_d_zero = 0;
    uint32_t export_epoch = 0;                      // W3_OPT_EXPORT_EPOCH (0 = W3_EXP_EPOCH_DEFAULT)
    w3_export_entropy_profile exp_prof{};           // (w3_export_get_profile returns its base)
    // ... for OrderNEntropy leaves (w3_export_entropy.h): the keys of one epoch, the Huffman key stage's state words
    DevBuf exp_k, exp_hs;
    // the per-step statistics export (w3_steps.h): the stream copies the row kernel reads (a single leaf's, before an APM stage rewrites it in
    // place, and every stage's but the last), the staged form's rows, the zero count of a caller's stream; what the last call did
    DevBuf steps_copies, steps_rows, probs_res;
    w3_steps_profile steps_prof{};
    uint64_t crc_res[2] = {~0ull, 0};
    // What a job takes from the context when a call is prepared (hand_options): the two-phase options (w3_ctx_set_option), the
    // context-mixing look-up tables in cm_luts, and the lane-order self-test's verdict (-1 not run yet under this variant, 1 = returning
    // LDS adds are lane-ordered, 0 = not: ballot rounds).
    TwoPhaseOptions opt;
    const int16_t *stretch = nullptr; const uint16_t *squash = nullptr; const uint2 *st = nullptr;
    int lds_order = -1;
    Job jobs[W3_MAX_JOBS];
    w3_ctx() { for (int j = 0; j < W3_MAX_JOBS; j++) jobs[j].index = j; }
    hipStream_t s_pred = nullptr, s_code[W3_MAX_JOBS] = {};   // created by the first w3_encode_submit
    int next_job = 0, last_job = -1;
    bool pooled_streams = false;
    hipStream_t s_side = nullptr, s_verify[W3_MAX_JOBS] = {};   // the workspaces' side stream (one: predict phases never overlap) and re-prediction streams
    // sharded calls in flight (w3_encode_sharded_submit / w3_encode_sharded_wait): this context's shard of step `slot`, in staging
    // buffers of its own until the step is gathered
    struct ShardSlot { int state = 0, djob = -1; DevBuf out, lens, total; size_t nb = 0, cap = 0; KeptCall call; } ss[W3_MAX_JOBS];
    // host-buffer calls in flight (w3_encode_host_submit / w3_encode_host_wait; w3_encode_blocks cuts its input into such calls)
    HostJob hj[W3_MAX_HOST_JOBS];
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;   // where the copies go: the context's stream, or (W3_OPT_TUNE bit 16) the two below
    hipStream_t s_h2d_own = nullptr, s_d2h_own = nullptr;
    uint64_t hseq = 0;
    uint32_t host_chunk_blocks = 0;                 // W3_OPT_HOST_CHUNK_BLOCKS (0 = auto)
    uint32_t aoh_batch_blocks = 0;                  // W3_OPT_AOH_BATCH_BLOCKS (0 = from the memory budget)
    // the sampled verification's rotation (w3_verify.h): a number per call, counted per input shape, whichever job slot the call lands
    // on; vcall_pin >= 0: the number the call being made now takes (a redo, or a piece of a host call) instead of a new one
    w3::VerifyCalls vcalls;
    int64_t vcall_pin = -1;
};

static uint64_t verify_call(w3_ctx *ctx, size_t n, size_t block_size) {
    return ctx->vcall_pin >= 0 ? (uint64_t)ctx->vcall_pin : ctx->vcalls.next(n, block_size);
}
// for the duration of a scope, calls take the number `v` (the number in effect before is restored afterwards)
struct VcallPin {
    w3_ctx *c; int64_t saved;
    VcallPin(w3_ctx *c_, uint64_t v) : c(c_), saved(c_->vcall_pin) { c->vcall_pin = (int64_t)v; }
    ~VcallPin() { c->vcall_pin = saved; }
};

#define HIPCHK(ctx, expr)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
            return W3_E_HIP;                                                                    \
        }                                                                                       \
    } while (0)

static int ensure(w3_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap && b.p) return W3_OK;
    if (b.p) { HIPCHK(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    size_t want = std::max<size_t>(bytes, 256);
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        ctx->err = "hipMalloc(" + std::to_string(want) + "): " + hipGetErrorString(e);
        (void)hipGetLastError();
        return W3_E_NOMEM;
    }
    b.cap = want;
    return W3_OK;
}
#define ENSURE(ctx, buf, bytes) do { int r_ = ensure(ctx, buf, bytes); if (r_) return r_; } while (0)

// Every entry point but w3_encode_submit / w3_encode_wait (and their host-buffer forms) works on job 0's workspace and the context's
// options: none of them may run while a submitted call is in flight (include/w3hip.h).
static int jobs_idle(w3_ctx *ctx) {
    for (const auto &J : ctx->jobs)
        if (J.state == 1) { ctx->err = "asynchronous jobs are in flight on this context: w3_encode_wait them first"; return W3_E_INVALID; }
    for (const auto &h : ctx->hj)
        if (h.state != 0) { ctx->err = "host-buffer jobs are in flight on this context: w3_encode_host_wait them first"; return W3_E_INVALID; }
    for (const auto &x : ctx->ss)
        if (x.state != 0) { ctx->err = "sharded jobs are in flight on this context: w3_encode_sharded_wait them first"; return W3_E_INVALID; }
    return W3_OK;
}

extern "C" int w3_abi_version(void) { return W3_ABI_VERSION; }

extern "C" const char *w3_strerror(int code) {
    switch (code) {
    case W3_OK: return "ok";
    case W3_E_INVALID: return "invalid argument or malformed model spec";
    case W3_E_NOSPACE: return "output buffer too small";
    case W3_E_HIP: return "HIP runtime error";
    case W3_E_UNSUPPORTED: return "model spec not implemented on the device";
    case W3_E_NOMEM: return "device workspace does not fit";
    case W3_E_FORMAT: return "bad container magic";
    case W3_E_CORRUPT: return "decoded block does not match its CRC-32";
    default: return "unknown error";
    }
}

extern "C" const char *w3_last_error(const w3_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

// The pipeline's streams are kept for the life of the process and handed from context to context (per device and priority): HIP deals
// hardware queues out when a stream is CREATED, by the queues' reference counts at that moment, and a context created after others
// had come and gone got code streams that shared queues (bench.py's later lines ran at the two-in-flight rate with four in flight).
struct StreamPool {
    std::mutex mu;
    std::vector<std::pair<long, hipStream_t>> idle;   // key = device * 8 + class (0 = predict, 1 = code, 2 = side, 3 = verification, 4 = the context's own launch / copy stream)
    hipStream_t take(long key) {
        std::lock_guard<std::mutex> g(mu);
        for (size_t i = 0; i < idle.size(); i++)
            if (idle[i].first == key) { hipStream_t s = idle[i].second; idle.erase(idle.begin() + (long)i); return s; }
        return nullptr;
    }
    void give(long key, hipStream_t s) { std::lock_guard<std::mutex> g(mu); idle.emplace_back(key, s); }
};
static StreamPool &stream_pool() { static StreamPool *p = new StreamPool; return *p; }   // (never destroyed: streams outlive static teardown order)

extern "C" int w3_ctx_create(int device, w3_ctx **out) {
    if (!out) return W3_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return W3_E_HIP;
    if (hipSetDevice(device) != hipSuccess) return W3_E_HIP;
    w3_ctx *c = new w3_ctx();
    c->device = device;
    // A BLOCKING stream: it is ordered against the legacy default (NULL) stream like any ordinary stream, so a caller that
    // produces d_in on the default stream and passes stream = NULL (or torch's default-stream handle, which is 0) gets the
    // order it expects.  The side streams of the predict phase fork from and join the launch stream with events.
    // Taken from the process-wide pool like the pipeline's streams: the host-buffer calls put their PCIe copies on this stream, and a
    // stream created after other contexts have come and gone can land on the hardware queue of a (pooled, still living) predict stream —
    // every copy then holds that call's kernels back (measured: 84.5 ms per 1e9-byte call in flight inside bench.py, where two contexts
    // had lived before, against 71.0 in a fresh process).
    c->stream = stream_pool().take(device * 8L + 4);
    if (!c->stream && hipStreamCreate(&c->stream) != hipSuccess) { delete c; return W3_E_HIP; }
    for (auto &e : c->jobs[0].ev)   // (a synchronous call can be timed; the other jobs' are created with the pipeline)
        if (hipEventCreate(&e) != hipSuccess) { delete c; return W3_E_HIP; }
    *out = c;
    return W3_OK;
}

extern "C" void w3_ctx_destroy(w3_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    DevBuf *bufs[] = {&ctx->tables, &ctx->lens, &ctx->total, &ctx->io_in, &ctx->io_out, &ctx->coffs, &ctx->misc, &ctx->cm_luts, &ctx->achash_luts,
                      &ctx->sweep, &ctx->aoh, &ctx->rg_stage, &ctx->rg_meta, &ctx->crc_ws, &ctx->crc_tab, &ctx->prep_ws,
                      &ctx->exp_d, &ctx->exp_s, &ctx->exp_list, &ctx->exp_stats, &ctx->exp_k, &ctx->exp_hs};
    for (DevBuf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    if (ctx->h_rg) (void)hipHostFree(ctx->h_rg);
    for (auto &J : ctx->jobs) {
        J.tp.release();
        for (DevBuf *b : {&J.stripes, &J.flag, &J.bits, &J.offs, &J.huff})
            if (b->p) (void)hipFree(b->p);
        for (auto &e : J.ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {J.ev_done, J.ev_in, J.ev_a, J.ev_apm}) if (e) (void)hipEventDestroy(e);
        if (J.h_status) (void)hipHostFree(J.h_status);
    }
    if (ctx->s_side) stream_pool().give(ctx->device * 8L + 2, ctx->s_side);
    for (auto &sv : ctx->s_verify) if (sv) stream_pool().give(ctx->device * 8L + 3, sv);
    if (ctx->pooled_streams) {   // (idle by now: the device was synchronised above)
        if (ctx->s_pred) stream_pool().give(ctx->device * 8L, ctx->s_pred);
        for (auto &sc : ctx->s_code) if (sc) stream_pool().give(ctx->device * 8L + 1, sc);
    } else {
        if (ctx->s_pred) (void)hipStreamDestroy(ctx->s_pred);
        for (auto &sc : ctx->s_code) if (sc) (void)hipStreamDestroy(sc);
    }
    for (auto &x : ctx->ss) {
        DevBuf *bufs3[] = {&x.out, &x.lens, &x.total};
        for (DevBuf *b : bufs3)
            if (b->p) (void)hipFree(b->p);
    }
    for (auto &h : ctx->hj) {
        DevBuf *bufs2[] = {&h.d_in, &h.d_out, &h.d_lens, &h.d_total};
        for (DevBuf *b : bufs2)
            if (b->p) (void)hipFree(b->p);
        if (h.ev_d2h) (void)hipEventDestroy(h.ev_d2h);
    }
    if (ctx->s_h2d_own) (void)hipStreamDestroy(ctx->s_h2d_own);
    if (ctx->s_d2h_own) (void)hipStreamDestroy(ctx->s_d2h_own);
    if (ctx->stream) stream_pool().give(ctx->device * 8L + 4, ctx->stream);   // (idle: the device was synchronised above)
    delete ctx;
}

extern "C" int w3_ctx_set_option(w3_ctx *ctx, int opt, int64_t value) {
    if (!ctx) return W3_E_INVALID;
    // A job in flight has taken its paths, variants and coder from the options: changing them between its predict and code stages would
    // mix two settings in one call.  Two options are exempt: W3_OPT_TIMING (read when a call is submitted) and W3_OPT_TUNE (scheduling
    // only: the output is identical whatever is set).
    if (opt != W3_OPT_TIMING && opt != W3_OPT_TUNE) { const int rc_ = jobs_idle(ctx); if (rc_) return rc_; }
    switch (opt) {
    case W3_OPT_PATH:
        if (value < W3_PATH_AUTO || value > W3_PATH_TWOPHASE) return W3_E_INVALID;
        ctx->opt_path = (int)value;
        return W3_OK;
    case W3_OPT_TIMING: ctx->opt_timing = value ? 1 : 0; return W3_OK;
    case W3_OPT_CODER:
        if (value < 0 || value > 5) return W3_E_INVALID;
        ctx->opt.coder_mode = (int)value;
        return W3_OK;
    case W3_OPT_DEBUG_STAMPS: ctx->opt.debug_stamps = value ? 1 : 0; return W3_OK;
    case W3_OPT_ACC_LIMIT:
        if (value < 19 || value > 46) return W3_E_INVALID;
        ctx->opt.acc_limit = (uint32_t)value;
        return W3_OK;
    case W3_OPT_VARIANT:
        if (value < 0 || value > 8191) return W3_E_INVALID;
        // the fault-injection hook exists for the test of the sampled verification: without the verification it would only corrupt output
        if ((value & W3_VAR_INJECT_LDS_FAULT) && !ctx->opt.verify) { ctx->err = "W3_OPT_VARIANT bit 32 (fault injection) needs W3_OPT_VERIFY on"; return W3_E_INVALID; }
        ctx->opt.variant = (uint32_t)value;
        ctx->lds_order = -1;   // re-run the lane-order self-test under the new setting
        return W3_OK;
    case W3_OPT_VERIFY:
        if (!value && (ctx->opt.variant & W3_VAR_INJECT_LDS_FAULT)) { ctx->err = "W3_OPT_VERIFY cannot be switched off while the fault-injection variant is set"; return W3_E_INVALID; }
        if (value < 0 || value > 256) return W3_E_INVALID;
        ctx->opt.verify = (int)value;   // 0 = off, v >= 1: v / 256 of the blocks are re-predicted per call (twophase_verify)
        return W3_OK;
    case W3_OPT_SLOT_BUDGET_MB:
        if (value < 0 || value > (1 << 20)) return W3_E_INVALID;
        ctx->opt.slot_budget_mb = (uint32_t)value;
        return W3_OK;
    case W3_OPT_TUNE:
        if (value < 0 || value > 0x1FFFFF) return W3_E_INVALID;
        ctx->opt.tune = (uint32_t)value;
        return W3_OK;
    case W3_OPT_FAULT_BLOCK:
        if (value < -1 || value > 0x7FFFFFFF) return W3_E_INVALID;
        ctx->opt.fault_block = value < 0 ? 0xFFFFFFFFu : (uint32_t)value;
        return W3_OK;
    case W3_OPT_FAULT_KERNELS:
        if (value < 1 || value > 7) return W3_E_INVALID;
        ctx->opt.fault_kernels = (uint32_t)value;
        return W3_OK;
    case W3_OPT_HOST_CHUNK_BLOCKS:
        if (value < 0 || value > 0x7FFFFFFF) return W3_E_INVALID;
        ctx->host_chunk_blocks = (uint32_t)value;
        return W3_OK;
    case W3_OPT_AOH_BATCH_BLOCKS:
        if (value < 0 || value > 0x7FFFFFFF) return W3_E_INVALID;
        ctx->aoh_batch_blocks = (uint32_t)value;
        return W3_OK;
    case W3_OPT_WAVE_GRID:
        if (value < 0 || value > 0x7FFFFFFF) return W3_E_INVALID;
        ctx->opt.wave_grid = (uint32_t)value;
        return W3_OK;
    case W3_OPT_EXPORT_EPOCH:
        if (value < 0 || value > (int64_t)W3_EXP_EPOCH_MAX || value % 1024) { ctx->err = "an export epoch is a multiple of 1 KiB, at most 2^28 bytes"; return W3_E_INVALID; }
        ctx->export_epoch = (uint32_t)value;
        return W3_OK;
    default: return W3_E_INVALID;
    }
}

extern "C" int w3_get_timing(const w3_ctx *ctx, w3_timing *out) {
    if (!ctx || !out) return W3_E_INVALID;
    *out = ctx->timing;
    return W3_OK;
}

// Hard bound: Counter probabilities lie in [1, 65535] so one bit-step costs at
// most 16 output bits (SURVEY §7 hard part 4): 16 bytes per input byte, plus
// the flush byte(s) per block.
extern "C" size_t w3_max_compressed_size(size_t n, size_t block_size) {
    if (block_size == 0) return 0;
    size_t nb = (n + block_size - 1) / block_size;
    return 16 * n + 8 * nb;
}

// ---------------------------------------------------------------------------
// model spec -> ordered leaf list
// ---------------------------------------------------------------------------
static int parse_spec(const w3_model_spec *spec, ParsedSpec &ps) {
    if (!spec || spec->n_nodes == 0 || spec->n_nodes > W3_MAX_NODES) return W3_E_INVALID;
    if (spec->n_huff > W3_MAX_HUFF || (spec->n_huff && !spec->huff)) return W3_E_INVALID;   // (the spec must be zero-initialised: w3hip.h)
    int depth = 0;
    bool plain_leaves = true;   // every subtree on the stack is a single adaptive leaf (what a W3_NODE_MIX can pop)
    uint32_t huff_used = 0;   // table sets some W3_HIST_HUFF leaf refers to: only those are read
    ps = ParsedSpec();
    for (uint32_t i = 0; i < spec->n_nodes; i++) {
        const w3_node &nd = spec->nodes[i];
        if (nd.kind == W3_NODE_APM) {
            // APM(model): one input.  Implemented as a chain at the root of the tree only.
            if (depth < 1 || nd.align > W3_APM_ORDER1 || nd.max_bits < 1 || nd.max_bits > 15) return W3_E_INVALID;
            if (depth != 1) return W3_E_UNSUPPORTED;
            if (ps.n_apm == W3_MAX_APM) return W3_E_UNSUPPORTED;
            ps.apm[ps.n_apm++] = nd;
            continue;
        }
        if (nd.kind == W3_NODE_MIX) {
            // logistic mixer over the N preceding single leaves (include/w3hip.h): the one mixer of the spec, over all its leaves
            if (!mix_params_ok(nd.bits, nd.align, nd.max_bits) || nd.history || nd.frozen || nd.log_cells || nd.reserved) return W3_E_INVALID;
            for (int k = 0; k < 8; k++)
                if (nd.table[k]) return W3_E_INVALID;
            if (ps.has_mix || ps.n_apm) return W3_E_UNSUPPORTED;   // a second mixer, a mixer behind an APM stage: valid, not built
            if (depth < (int)nd.bits) return W3_E_INVALID;
            if (!plain_leaves || depth != (int)nd.bits) return W3_E_UNSUPPORTED;   // BestOfTwo / frozen leaves under it, leaves beside it
            ps.has_mix = true; ps.mix = nd;
            depth = 1;
            continue;
        }
        if (ps.n_apm || ps.has_mix) return nd.kind == W3_NODE_ORDERN || nd.kind == W3_NODE_SLOT_STATE || nd.kind == W3_NODE_BEST_OF_TWO ? W3_E_UNSUPPORTED : W3_E_INVALID;
        if (nd.kind == W3_NODE_ORDERN) {
            // OrderN::new allocates 1<<bits counters; masks are u32/u8 (ordern.rs:35-43)
            if (nd.bits < 1 || nd.bits > 32 || nd.align > 7 || nd.align > nd.bits) return W3_E_INVALID;
            if ((int)nd.bits - (int)nd.align > 31) return W3_E_INVALID;
            if (nd.history > W3_HIST_MATCH) return W3_E_INVALID;
            if (nd.history == W3_HIST_AC && nd.max_bits > 32) return W3_E_INVALID;
            if (nd.history == W3_HIST_MATCH) {   // MatchHistory(min_len = max_bits, log_slots = log_cells): w3_match_plan.h
                if (!match_params_ok(nd.max_bits, nd.log_cells)) return W3_E_INVALID;
                if (nd.bits != MATCH_BITS || nd.align != MATCH_ALIGN) return W3_E_UNSUPPORTED;
                if (ps.has_match) return W3_E_UNSUPPORTED;   // a second match leaf: valid, not built
                ps.has_match = true;
            }
            if (nd.history == W3_HIST_HUFF) {
                if (nd.reserved >= spec->n_huff) return W3_E_INVALID;
                huff_used |= 1u << nd.reserved;
            }
            if (ps.n_leaves == W3_MAX_LEAVES) return W3_E_UNSUPPORTED;
            ps.leaf[ps.n_leaves++] = nd;
            plain_leaves &= !nd.frozen;
            depth++;
        } else if (nd.kind == W3_NODE_SLOT_STATE) {
            if (nd.bits > 7 || nd.log_cells < 1 || nd.log_cells > 24 || nd.frozen) return W3_E_INVALID;
            if (ps.n_leaves == W3_MAX_LEAVES) return W3_E_UNSUPPORTED;
            ps.leaf[ps.n_leaves++] = nd;
            ps.has_slot = true;
            depth++;
        } else if (nd.kind == W3_NODE_BEST_OF_TWO) {
            if (depth < 2) return W3_E_INVALID;
            plain_leaves = false;
            depth--;
        } else {
            return W3_E_INVALID;
        }
    }
    // the table sets travel to the device only when a leaf uses one (a spec without HuffHistory leaves never has its huff
    // pointer dereferenced); code lengths index shifts of u32 values
    ps.n_huff = huff_used ? spec->n_huff : 0;
    ps.huff = ps.n_huff ? spec->huff : nullptr;
    for (uint32_t k = 0; k < ps.n_huff; k++) {
        if (!((huff_used >> k) & 1u)) continue;
        for (int v = 0; v < 256; v++)
            if (ps.huff[k].len[v] > 16 || ps.huff[k].rem_len[v] > 16) return W3_E_INVALID;
    }
    return depth == 1 ? W3_OK : W3_E_INVALID;
}

// HuffHistory table sets of the spec -> device (per call: the tables are the caller's memory); job 0's copy, which is where the
// lane-per-block kernels (they run on job 0 only) find them
static int stage_huff(w3_ctx *ctx, hipStream_t s, const ParsedSpec &ps);
static const w3_huff_table *lane_huff(const w3_ctx *ctx, const ParsedSpec &ps) { return ps.n_huff ? (const w3_huff_table *)ctx->jobs[0].huff.p : nullptr; }

extern "C" int w3_spec_validate(const w3_model_spec *spec) {
    ParsedSpec ps;
    return parse_spec(spec, ps);
}

// Lay out the per-lane model tables of the generic path.
static uint64_t layout_generic(const ParsedSpec &ps, size_t block_size, GenericArgs &ga) {
    uint64_t off = 0;
    ga.n_leaves = ps.n_leaves;
    for (int l = 0; l < ps.n_leaves; l++) {
        const w3_node &nd = ps.leaf[l];
        LeafParam &lp = ga.leaf[l];
        memset(&lp, 0, sizeof lp);
        lp.bits = nd.bits; lp.align = nd.align; lp.hist = nd.history; lp.max_bits = nd.max_bits; lp.frozen = nd.frozen;
        lp.huff_idx = nd.history == W3_HIST_HUFF ? nd.reserved : 0;
        memcpy(lp.table, nd.table, sizeof lp.table);
        lp.tbl_off = off;
        if (nd.kind == W3_NODE_SLOT_STATE) {   // HashMap of 2^log_cells 96-byte Cells (hashmap.rs:7-22)
            lp.kind = 1; lp.order = nd.bits; lp.log_cells = nd.log_cells;
            off += 96ull << nd.log_cells;
            continue;
        }
        lp.hist_mask = (uint32_t)((1ull << (nd.bits - nd.align)) - 1ull);
        if (nd.frozen) continue;
        if (nd.history == W3_HIST_MATCH) {   // T_m and T_2m, 2^L u32 each, right BEFORE the leaf's Counter table (match_tables, w3_generic.h)
            lp.log_cells = nd.log_cells;
            off += 8ull << nd.log_cells;
            lp.tbl_off = off;
        }
        const CounterTable t = counter_table(nd.bits, (uint64_t)block_size * 8);
        lp.use_hash = t.use_hash; lp.hash_mask = t.use_hash ? (uint32_t)(t.slots - 1) : 0u;
        off += t.use_hash ? t.hash_bytes : t.direct_bytes;
    }
    return std::max<uint64_t>(off, 16);
}

// ACHistory leaves of the lane-per-block kernels: tabulate the coder states of every 16-bit history prefix once per call
// (k_achash_lut, w3_predict.h) so that leaf_ctx looks the hash up instead of running the nested coder bit by bit.
static int prepare_achash_luts(w3_ctx *ctx, hipStream_t s, GenericArgs &ga);

// the decoders' length table: enqueue the exclusive scan of d_lens[nb] into ctx->coffs, its sum into ctx->total
static int scan_lens(w3_ctx *ctx, hipStream_t s, const uint32_t *d_lens, uint32_t nb) {
    ENSURE(ctx, ctx->coffs, (size_t)nb * 8);
    ENSURE(ctx, ctx->total, 8);
    hipLaunchKernelGGL(k_scan_lens, dim3(1), dim3(1024), 0, s, d_lens, (uint64_t *)ctx->coffs.p, (uint64_t *)ctx->total.p, nb);
    return W3_OK;
}
// ... and the table must not claim more than the caller's buffer holds: the kernels read cin + offset for clens[b] bytes
static int check_len_table(w3_ctx *ctx, hipStream_t s, const uint32_t *d_lens, uint32_t nb, size_t in_len) {
    if (const int rc = scan_lens(ctx, s, d_lens, nb)) return rc;
    uint64_t total = 0;
    HIPCHK(ctx, hipMemcpyAsync(&total, ctx->total.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (total > in_len) { ctx->err = "block length table claims " + std::to_string(total) + " compressed bytes, the buffer holds " + std::to_string(in_len); return W3_E_FORMAT; }
    return W3_OK;
}

// ---------------------------------------------------------------------------
// pack: scan block lengths, compact stripes into d_out
// ---------------------------------------------------------------------------
static int run_pack(w3_ctx *ctx, Job &J, hipStream_t s, const uint8_t *stripes, uint64_t stride, const uint32_t *d_lens, uint32_t nb,
                    uint8_t *d_out, size_t out_cap, uint64_t *d_total) {
    ENSURE(ctx, J.offs, (size_t)nb * 8);
    hipLaunchKernelGGL(k_scan_lens, dim3(1), dim3(1024), 0, s, d_lens, (uint64_t *)J.offs.p, d_total, nb);
    uint32_t grid = std::min<uint32_t>(nb, 256 * 8);
    hipLaunchKernelGGL(k_pack, dim3(grid), dim3(256), 0, s, stripes, stride, d_lens, (const uint64_t *)J.offs.p, d_out,
                       (uint64_t)out_cap, nb);
    HIPCHK(ctx, hipGetLastError());
    return W3_OK;
}

// ---------------------------------------------------------------------------
// lane-per-block path (w3_generic.h, w3_cm.h): every spec, encode and decode, through one runner (lane_run)
// ---------------------------------------------------------------------------
static int table_budget(w3_ctx *ctx, uint64_t lane_stride, uint32_t want_lanes, uint32_t &lanes_out) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    // (Every block of a call resident at once matters to the decoders: they are latency chains per block, so two batches take twice as
    // long as one.  The default model's tables are 10 MiB per block = 153 GB at enwik9 size.)
    const uint64_t avail_b = (uint64_t)free_b + ctx->tables.cap;
    uint64_t budget = std::min<uint64_t>(avail_b > (12ull << 30) ? avail_b - (12ull << 30) : avail_b / 2, 224ull << 30);
    uint64_t lanes = budget / lane_stride;
    if (lanes >= want_lanes) lanes = want_lanes;
    else lanes = lanes / 64 * 64;
    if (lanes == 0) {
        ctx->err = "model tables of one wavefront (" + std::to_string(lane_stride * 64) + " B) exceed the device budget";
        return W3_E_NOMEM;
    }
    // One hipMalloc of that size can still fail (fragmentation, another process or rank on the same GPU, a caching allocator that
    // holds what hipMemGetInfo calls free): take half the lanes then — the callers run batches — rather than fail the call.
    for (;;) {
        const int rc = ensure(ctx, ctx->tables, (size_t)lanes * lane_stride);
        if (rc == W3_OK) break;
        if (rc != W3_E_NOMEM || lanes <= 64) return rc;
        lanes = std::max<uint64_t>(64, lanes / 2 / 64 * 64);
    }
    lanes_out = (uint32_t)lanes;
    return W3_OK;
}

static int prepare_achash_luts(w3_ctx *ctx, hipStream_t s, GenericArgs &ga) {
    int n_ac = 0;
    for (int l = 0; l < ga.n_leaves; l++) n_ac += ga.leaf[l].kind == 0 && ga.leaf[l].hist == W3_HIST_AC && !ga.leaf[l].frozen;
    if (!n_ac) return W3_OK;
    const size_t entries = (size_t)8u << W3_ACHASH_LUT_BITS, per_leaf = entries * 18;
    ENSURE(ctx, ctx->achash_luts, per_leaf * (size_t)n_ac);
    int k = 0;
    for (int l = 0; l < ga.n_leaves; l++) {
        LeafParam &lp = ga.leaf[l];
        if (!(lp.kind == 0 && lp.hist == W3_HIST_AC && !lp.frozen)) continue;
        uint8_t *base = (uint8_t *)ctx->achash_luts.p + per_leaf * (size_t)k++;
        HashArgs ha;
        memset(&ha, 0, sizeof ha);
        ha.max_bits = lp.max_bits; ha.hmask = 0xFFu;
        memcpy(ha.table, lp.table, sizeof ha.table);
        ha.lut = (uint4 *)base; ha.lut_key = (uint16_t *)(base + entries * 16);
        hipLaunchKernelGGL(k_achash_lut, dim3((unsigned)(entries / 256)), dim3(256), 0, s, ha);
        lp.lut = (const uint4 *)base;
    }
    HIPCHK(ctx, hipGetLastError());
    return W3_OK;
}

// k_decode_spec's group: the whole nibble.  Half a nibble (W3_OPT_TUNE bit 14: four lanes per block, 6 instead of 15 speculative look-ups per
// nibble and leaf) was measured for the large batches, which are bound by those look-ups' HBM traffic — order012apm 736 -> 758 MiB/s at 1e9 B,
// but order012 856 -> 778, Order0 3,906 -> 3,366, main.rs default 1,585 -> 1,417, and 189 -> 104 MiB/s at 1e8 B: four round trips per nibble
// instead of two, and a quarter of the wavefronts to hide them (profiles/r3_decode_spec/).  Kept as a tested variant.
static int decode_group_bits(const w3_ctx *ctx) { return (ctx->opt.tune & 16384u) ? 2 : 4; }

static int cm_luts(w3_ctx *ctx, hipStream_t s, CmArgs &ca) {
    const size_t st_bytes = (size_t)kStSize * 8, str_bytes = 4096 * 2, sq_bytes = 4096 * 2;
    if (!ctx->cm_luts.p) {
        ENSURE(ctx, ctx->cm_luts, st_bytes + str_bytes + sq_bytes);
        std::vector<StEntry> t(kStSize);
        build_state_table(t.data());
        std::vector<uint32_t> packed(2 * kStSize);
        for (int i = 0; i < kStSize; i++) {
            packed[2 * i] = t[i].prob | ((uint32_t)t[i].next0 << 16);
            packed[2 * i + 1] = t[i].next1 | ((uint32_t)t[i].conf << 16);
        }
        std::vector<int16_t> str(4096);
        std::vector<uint16_t> sq(4096);
        build_stretch_squash(str.data(), sq.data());
        uint8_t *d = (uint8_t *)ctx->cm_luts.p;
        HIPCHK(ctx, hipMemcpy(d, packed.data(), st_bytes, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(d + st_bytes, str.data(), str_bytes, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(d + st_bytes + str_bytes, sq.data(), sq_bytes, hipMemcpyHostToDevice));
    }
    (void)s;
    uint8_t *d = (uint8_t *)ctx->cm_luts.p;
    ca.st = (const uint2 *)d;
    ca.stretch = (const int16_t *)(d + st_bytes);
    ca.squash = (const uint16_t *)(d + st_bytes + str_bytes);
    return W3_OK;
}

// The per-lane table region: the Counter tables and slot-leaf hash maps (layout_generic), then, for specs with APM stages or slot
// leaves, rounded up to 16 bytes, the APM tables and the logistic mixer's weights.  Returns the lane stride.
static uint64_t layout_lane(const ParsedSpec &ps, size_t block_size, CmArgs &ca) {
    uint64_t off = layout_generic(ps, block_size, ca.g);
    if (!ps.is_cm()) return off;
    off = (off + 15) / 16 * 16;
    ca.n_apm = ps.n_apm;
    for (int k = 0; k < ps.n_apm; k++) {
        ca.apm[k].ctx_kind = ps.apm[k].align;
        ca.apm[k].rate = ps.apm[k].max_bits;
        ca.apm[k].off = off;
        // (272 rows per page of 256: k_decode_spec keeps the table nibble-major, 17 groups of 16 node columns — w3_decode_spec.h)
        off += ((ps.apm[k].align == W3_APM_ORDER1 ? 256ull : 1ull) * 272 * 33 * 2 + 15) / 16 * 16;
    }
    if (ps.has_mix) {   // the mixer's weights int32[S][N], behind the APM tables
        ca.mix.n = ps.mix.bits; ca.mix.select = ps.mix.align; ca.mix.rate = ps.mix.max_bits;
        ca.mix.off = off;
        off += ((uint64_t)mix_sets(ps.mix.align) * ps.mix.bits * 4 + 15) / 16 * 16;
    }
    return off;
}

// Which lane-per-block kernel runs a spec, over cnt lanes.  Up to 4 Counter leaves and no slot leaves: the kernels with all Counter
// loads of a step in flight together, k_generic_nl without and k_cm_nl with an APM chain.  Otherwise the run-time leaf loop: without
// APM stages and slot leaves k_generic, else the slot cells staged in LDS (k_cm_staged: up to W3_CM_STAGED_MAX slot leaves, none
// included) or in global memory (k_cm).  Specs of Counter leaves alone take the kernels over GenericArgs, the rest those over CmArgs.
template <bool DECODE>
static void lane_launch(const CmArgs &ca, uint32_t cnt, hipStream_t s, bool unstaged) {
    static void (*const plain_nl[4])(GenericArgs) = {k_generic_nl<DECODE, 1>, k_generic_nl<DECODE, 2>, k_generic_nl<DECODE, 3>, k_generic_nl<DECODE, 4>};
    static void (*const cm_nl[4])(CmArgs) = {k_cm_nl<DECODE, 1>, k_cm_nl<DECODE, 2>, k_cm_nl<DECODE, 3>, k_cm_nl<DECODE, 4>};
    const dim3 grid((cnt + 63) / 64), blk(64);
    const int nl = ca.g.n_leaves;
    int n_slot = 0;
    for (int l = 0; l < nl; l++) n_slot += ca.g.leaf[l].kind == 1;
    bool match = false;
    for (int l = 0; l < nl; l++) match |= ca.g.leaf[l].kind == 0 && ca.g.leaf[l].hist == W3_HIST_MATCH && !ca.g.leaf[l].frozen;   // (frozen: no context is ever formed)
    if (match) {   // a match-model leaf: the run-time leaf loops with the MATCH flag (never the _nl forms), with or without a mixer
        if (!n_slot && !ca.n_apm && !ca.mix.n) { hipLaunchKernelGGL((k_generic<DECODE, true>), grid, blk, 0, s, ca.g); return; }
        void (*const staged)(CmArgs) = ca.mix.n ? k_cm_staged<DECODE, true, true> : k_cm_staged<DECODE, false, true>;
        void (*const plain)(CmArgs) = ca.mix.n ? k_cm<DECODE, true, true> : k_cm<DECODE, false, true>;
        hipLaunchKernelGGL(n_slot <= W3_CM_STAGED_MAX && !unstaged ? staged : plain, grid, blk, 0, s, ca);
        return;
    }
    if (ca.mix.n) {   // a logistic mixer over the leaves: the run-time leaf loops, by the same staged rule (never k_cm_nl / k_generic*)
        void (*const staged)(CmArgs) = k_cm_staged<DECODE, true>, (*const plain)(CmArgs) = k_cm<DECODE, true>;
        hipLaunchKernelGGL(n_slot <= W3_CM_STAGED_MAX && !unstaged ? staged : plain, grid, blk, 0, s, ca);
        return;
    }
    const bool batch = !n_slot && nl >= 1 && nl <= 4;
    if (!n_slot && !ca.n_apm) hipLaunchKernelGGL(batch ? plain_nl[nl - 1] : k_generic<DECODE>, grid, blk, 0, s, ca.g);
    else hipLaunchKernelGGL(batch ? cm_nl[nl - 1] : n_slot <= W3_CM_STAGED_MAX && !unstaged ? k_cm_staged<DECODE> : k_cm<DECODE>, grid, blk, 0, s, ca);
}

// What one call of the lane-per-block path codes.  Encode: in -> job 0's stripes of stripe_cap bytes each, the blocks' lengths to out_len.
// Decode: the streams cin, by the length table clens[nb], -> dout: every block whole (jobs == nullptr), or the n_jobs decode jobs (the
// random-access decode: w3_ranges.h) — the lanes, and with them the table budget's batches, the table zero-fill, the APM tables'
// initialisation and k_decode_spec's choices, then count jobs instead of blocks.
// Decode precondition: ctx->coffs holds the exclusive scan of clens[nb], enqueued on s (scan_lens / check_len_table).
struct LaneIo {
    const uint8_t *in = nullptr; uint32_t stripe_cap = 0; uint32_t *out_len = nullptr;
    const uint8_t *cin = nullptr; const uint32_t *clens = nullptr; uint8_t *dout = nullptr; const DecodeJob *jobs = nullptr; uint32_t n_jobs = 0;
};

// Does a decode take k_decode_spec?  Where the kernel covers the spec (decode_spec_covers), unless the lane kernels are asked for by name
// (W3_VAR_DECODE_LANE: the cross-check) — and, for a spec with a logistic mixer, only with nibble groups: the two-bit-group variant
// (decode_group_bits) is not built for it.  A spec with a live match-model leaf is taken only where W3_VAR_DECODE_MATCH_SPEC asks for it
// (the MATCH instances of k_decode_spec; the default stays the lane kernels), and it too only with nibble groups.  One rule for the launch,
// the APM tables' format (nm_tables below), w3_decode_spec_covers and w3_decode_spec_covers_variant.
static bool decode_takes_spec(const CmArgs &ca, uint32_t variant, int group_bits) {
    if (!decode_spec_covers(ca, (variant & W3_VAR_DECODE_MATCH_SPEC) != 0) || (variant & W3_VAR_DECODE_LANE)) return false;
    return !((ca.mix.n || decode_spec_has_match(ca)) && group_bits != 4);
}

template <bool DECODE>
static int lane_run(w3_ctx *ctx, hipStream_t s, const ParsedSpec &ps, size_t block_size, uint64_t n, uint32_t nb, const LaneIo &io) {
    CmArgs ca;
    memset(&ca, 0, sizeof ca);
    GenericArgs &g = ca.g;
    const uint64_t lane_stride = layout_lane(ps, block_size, ca);
    const uint32_t nl = io.jobs ? io.n_jobs : nb;   // (the lanes: blocks, or jobs)
    uint32_t lanes = 0;
    int rc = table_budget(ctx, lane_stride, nl, lanes);
    if (rc) return rc;
    if ((rc = prepare_achash_luts(ctx, s, g))) return rc;
    if (ps.is_cm() && (rc = cm_luts(ctx, s, ca))) return rc;
    ca.dflags = (ctx->opt.tune >> 17) & 7u;
    g.n = n; g.block_size = (uint32_t)block_size;
    g.huff = lane_huff(ctx, ps); g.n_huff = (int)ps.n_huff;
    g.tables = (uint8_t *)ctx->tables.p; g.lane_stride = lane_stride;
    if (DECODE) {
        g.cin = io.cin; g.coffs = (const uint64_t *)ctx->coffs.p; g.clens = io.clens; g.dout = io.dout; g.jobs = io.jobs;
    } else {
        g.in = io.in; g.stripe_cap = io.stripe_cap; g.out_len = io.out_len;
        g.overflow = (uint32_t *)ctx->jobs[0].flag.p; g.out_bits = (uint32_t *)ctx->jobs[0].bits.p;
    }
    // the nibble's context tree at once, sixteen lanes per block (w3_decode_spec.h), where it applies
    const bool spec_dec = DECODE && decode_takes_spec(ca, ctx->opt.variant, decode_group_bits(ctx));
    if (DECODE) ctx->last_decode_path = spec_dec ? W3_PATH_SPEC : W3_PATH_GENERIC;   // (w3_last_decode_path; w3_timing is an encode's record)
    for (uint32_t first = 0; first < nl; first += lanes) {
        const uint32_t cnt = std::min(lanes, nl - first);
        g.first_block = first; g.n_lanes = cnt;
        if (!DECODE) g.stripes = (uint8_t *)ctx->jobs[0].stripes.p + (uint64_t)first * io.stripe_cap;
        HIPCHK(ctx, hipMemsetAsync(ctx->tables.p, 0, (size_t)cnt * lane_stride, s));
        const bool nm_tables = spec_dec && decode_spec_nibble_major(ca, cnt, decode_group_bits(ctx));   // (the APM tables' layout follows the kernel's)
        for (int k = 0; k < ca.n_apm; k++)
            hipLaunchKernelGGL(k_cm_init_apm, dim3(2048), dim3(256), 0, s, g.tables, lane_stride, ca.apm[k].off,
                               nm_tables ? (ca.apm[k].ctx_kind ? 256u * 272u : 272u) : (ca.apm[k].ctx_kind ? 65536u : 256u), cnt, ca.squash, nm_tables ? 1u : 0u);
        if (ca.mix.n)
            hipLaunchKernelGGL(k_cm_init_mix, dim3(std::min<uint32_t>(2048u, (uint32_t)(((uint64_t)cnt * mix_sets(ca.mix.select) * ca.mix.n + 255) / 256))), dim3(256), 0, s,
                               g.tables, lane_stride, ca.mix.off, mix_sets(ca.mix.select) * ca.mix.n, cnt, mix_w_init(ca.mix.n));
        if (spec_dec) launch_decode_spec(ca, cnt, s, decode_group_bits(ctx));
        else lane_launch<DECODE>(ca, cnt, s, (ctx->opt.variant & W3_VAR_CM_UNSTAGED) != 0);
        HIPCHK(ctx, hipGetLastError());
    }
    return W3_OK;
}

extern "C" int w3_decode_spec_covers(const w3_model_spec *spec) {
    ParsedSpec ps;
    if (const int rc = parse_spec(spec, ps)) return rc;
    CmArgs ca;
    memset(&ca, 0, sizeof ca);
    layout_lane(ps, 65536, ca);   // (the leaves' kinds and alignments, the chain, the mixer: nothing the answer reads depends on the block size)
    return decode_takes_spec(ca, 0u, 4) ? 1 : 0;
}
extern "C" int w3_decode_spec_covers_variant(const w3_model_spec *spec, uint32_t variant) {
    ParsedSpec ps;
    if (const int rc = parse_spec(spec, ps)) return rc;
    CmArgs ca;
    memset(&ca, 0, sizeof ca);
    layout_lane(ps, 65536, ca);
    return decode_takes_spec(ca, variant, 4) ? 1 : 0;
}
extern "C" int w3_last_decode_path(const w3_ctx *ctx) { return ctx ? ctx->last_decode_path : 0; }
extern "C" int w3_last_wave_grid(const w3_ctx *ctx, uint32_t out[2]) {
    if (!ctx || !out) return W3_E_INVALID;
    out[0] = ctx->last_wave_grid[0]; out[1] = ctx->last_wave_grid[1];
    return W3_OK;
}

// ---------------------------------------------------------------------------
// encode (device-resident)
// ---------------------------------------------------------------------------
// Does an encode of this spec and shape take the two-phase path?  W3_PATH_GENERIC never, W3_PATH_TWOPHASE wherever the predict kernels
// cover the spec, W3_PATH_AUTO likewise — but for a spec with a logistic mixer node only where the mixer stage has been measured to beat
// the lane kernel (lmix_auto_twophase, w3_lmix.h).
static bool takes_twophase(const w3_ctx *ctx, const ParsedSpec &ps, size_t block_size, size_t n) {
    if (ctx->opt_path == W3_PATH_GENERIC || !twophase_supported(ps, block_size, n)) return false;
    if (ps.has_mix && ctx->opt_path == W3_PATH_AUTO) return lmix_auto_twophase((n + block_size - 1) / block_size, block_size);
    return true;
}

static uint32_t default_stripe_cap(size_t block_size) {
    // realistic bound 2N+64 (adaptive Counter regret is small); the exact bound 16N+8 is the retry size
    uint64_t c = 2 * (uint64_t)block_size + 64;
    return (uint32_t)((c + 15) / 16 * 16);
}
static uint32_t worst_stripe_cap(size_t block_size) {
    uint64_t c = 16 * (uint64_t)block_size + 16;
    return (uint32_t)((c + 15) / 16 * 16);
}

static int check_args(w3_ctx *ctx, size_t n, size_t block_size, bool one_device = true) {
    if (!ctx) return W3_E_INVALID;
    if (block_size == 0 || block_size > (1u << 28)) { ctx->err = "block_size must be in 1..2^28"; return W3_E_INVALID; }
    if ((n + block_size - 1) / block_size > 0x7FFFFFFFull) { ctx->err = "too many blocks"; return W3_E_INVALID; }
    // One call handles less than 4 GiB: the per-byte kernels are launched with one work-item per input byte, and a dispatch counts its
    // work-items in 32 bits (a larger launch would silently cover n mod 2^32 bytes).  Blocks are independent: larger inputs are split by the caller.
    if (one_device && n >= (1ull << 32) - 4096u) { ctx->err = "one call handles less than 4 GiB of input: split larger inputs at block boundaries (blocks are independent)"; return W3_E_UNSUPPORTED; }
    return W3_OK;
}

static float elapsed_ev(hipEvent_t *ev, int slot) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[2 * slot], ev[2 * slot + 1]) != hipSuccess) { (void)hipGetLastError(); return 0.f; }
    return ms;
}

// per-kernel launch times of one two-phase encode from its events (W3_OPT_TIMING)
static void collect_timing(hipEvent_t *ev, const TwoPhaseWs &ws, bool has_apm, bool has_slot, bool has_mix, bool packed, w3_timing &t) {
    t.predict_ms = elapsed_ev(ev, W3_EV_PREDICT); t.coder_ms = elapsed_ev(ev, W3_EV_CODER);
    if (has_apm) t.apm_ms = elapsed_ev(ev, W3_EV_APM);
    if (has_mix) t.mix_ms = elapsed_ev(ev, W3_EV_MIX);
    if (has_slot) t.slot_ms = elapsed_ev(ev, W3_EV_SLOT);
    if (ws.achash_timed) t.achash_ms = elapsed_ev(ev, W3_EV_ACHASH);
    t.n_wide = (uint32_t)std::min(ws.n_wide, 4);
    for (int w = 0; w < ws.n_wide && w < 4; w++) { t.part_ms[w] = elapsed_ev(ev, W3_EV_PART0 + w); t.rank_ms[w] = elapsed_ev(ev, W3_EV_RANK0 + w); }
    if (ws.small_timed) t.small_ms = elapsed_ev(ev, W3_EV_SMALL);
    if (ws.match_timed) t.match_ms = elapsed_ev(ev, W3_EV_MATCH);
    t.pack_ms = packed ? elapsed_ev(ev, W3_EV_PACK) : 0.f;
    t.total_ms = elapsed_ev(ev, W3_EV_TOTAL);
}

static int stage_huff_job(w3_ctx *ctx, Job &J, hipStream_t s, const ParsedSpec &ps) {
    J.tp.huff = nullptr;
    if (!ps.n_huff) return W3_OK;
    ENSURE(ctx, J.huff, sizeof(w3_huff_table) * W3_MAX_HUFF);
    HIPCHK(ctx, hipMemcpyAsync(J.huff.p, ps.huff, sizeof(w3_huff_table) * ps.n_huff, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s));   // (pageable source: the caller may free it after the call)
    J.tp.huff = (const w3_huff_table *)J.huff.p;
    return W3_OK;
}

static int stage_huff(w3_ctx *ctx, hipStream_t s, const ParsedSpec &ps) { return stage_huff_job(ctx, ctx->jobs[0], s, ps); }

// What the context owns reaches a job's workspace here, when a call is prepared: the options as one block, the look-up tables, and the
// lane-order self-test's verdict (one run per variant setting, on the workspace that asks first).
static void hand_options(w3_ctx *ctx, Job &J, bool two) {
    J.tp.opt = ctx->opt;
    if (J.index) J.tp.opt.debug_stamps = 0;   // (w3_debug_get_stamps reads job 0's)
    J.tp.stretch = ctx->stretch; J.tp.squash = ctx->squash; J.tp.st = ctx->st;
    J.tp.lds_order = ctx->lds_order;
    J.tp.last_wave_grid = ctx->last_wave_grid;
    if (two && ctx->lds_order < 0) { (void)twophase_lds_order_ok(J.tp, ctx->stream); ctx->lds_order = J.tp.lds_order; }
}

// The sampled verification saw the LDS-add rounds misbehave: this context codes with the ballot rounds from now on, on every slot.
static void use_ballot_rounds(w3_ctx *ctx) {
    ctx->opt.variant |= W3_VAR_NO_LDS_ATOMICS; ctx->lds_order = 0;
    for (auto &J : ctx->jobs) { J.tp.opt.variant |= W3_VAR_NO_LDS_ATOMICS; J.tp.lds_order = 0; }
}

// The side stream of the predict phase and the job's re-prediction stream: the context's (taken from the process-wide pool), so that
// a context does not create streams — and with them hardware-queue assignments — of its own for every workspace.
static int attach_aux_streams(w3_ctx *ctx, Job &J) {
    if (!ctx->s_side) {
        ctx->s_side = stream_pool().take(ctx->device * 8L + 2);
        if (!ctx->s_side) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->s_side, hipStreamNonBlocking));
    }
    hipStream_t &sv = ctx->s_verify[J.index];
    if (!sv) {
        sv = stream_pool().take(ctx->device * 8L + 3);
        if (!sv) {
            int lo_p = 0, hi_p = 0;
            HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&lo_p, &hi_p));
            HIPCHK(ctx, hipStreamCreateWithPriority(&sv, hipStreamNonBlocking, lo_p));
        }
    }
    J.tp.side = ctx->s_side; J.tp.vstream = sv; J.tp.ext_streams = true;
    return W3_OK;
}

static int stage_cm_luts(w3_ctx *ctx, hipStream_t s) {
    CmArgs lut;
    const int rc = cm_luts(ctx, s, lut);
    if (!rc) { ctx->stretch = lut.stretch; ctx->squash = lut.squash; ctx->st = lut.st; }
    return rc;
}

// Everything a call needs in job J before its first attempt, enqueued on s where it touches the device: the status and bit-count
// buffers, the spec's HuffHistory tables, the context-mixing look-up tables, the context's options, the side streams, the call's
// number for the verification's rotation and the places its kernels report to.  two: the call takes the two-phase path.  What repeats per attempt (stripes at the attempt's cap, cleared status words) is the caller's.
static int job_prepare(w3_ctx *ctx, Job &J, const ParsedSpec &ps, hipStream_t s, bool two, bool half_cu, size_t n, size_t block_size, uint32_t nb) {
    int rc;
    ENSURE(ctx, J.flag, 4 * ST_WORDS);
    ENSURE(ctx, J.bits, (size_t)nb * 4);
    if ((rc = stage_huff_job(ctx, J, s, ps))) return rc;
    if (two && ps.is_cm() && (rc = stage_cm_luts(ctx, s))) return rc;
    hand_options(ctx, J, two);
    if ((rc = attach_aux_streams(ctx, J))) return rc;
    J.tp.half_cu = half_cu;
    J.tp.verify_calls = verify_call(ctx, n, block_size);   // (counted per shape by the context: a call's job slot does not matter)
    J.tp.out_bits = (uint32_t *)J.bits.p;
    J.tp.order_fault = (uint32_t *)J.flag.p + ST_ORDER_FAULT;
#ifdef W3_TUNING
    J.tp.apm_oob = (uint32_t *)J.flag.p + ST_APM_OOB;
#endif
    return W3_OK;
}

// ctx->timing of a finished two-phase call: the launch statistics its enqueueing collected in ptm, and (timed calls) the event times
static void fill_timing(w3_ctx *ctx, Job &J, const w3_timing &ptm, uint64_t total, const ParsedSpec &ps, bool timed, bool packed) {
    ctx->timing.path = W3_PATH_TWOPHASE;
    ctx->timing.coder_bytes = ptm.coder_bytes + total; ctx->timing.predict_bytes = ptm.predict_bytes;
    ctx->timing.n_coder_launches = ptm.n_coder_launches; ctx->timing.n_slot_launches = ptm.n_slot_launches;
    ctx->timing.n_parts = 1;
    if (timed) collect_timing(J.ev, J.tp, ps.n_apm > 0, ps.has_slot, ps.has_mix, packed, ctx->timing);
}

// The attempts of one synchronous encode on job J (encode_core's, for a model's streams and for a caller's alike: the attempt is what
// differs between the two): `attempt(cap)` enqueues one attempt's kernels with stripes of `cap` bytes per block; its status words are
// read back, handed-back blocks are recoded, and the attempt is repeated on the ballot path or with the worst-case stripes where the words
// ask for it (w3_jobs.h).  cap: in = the first attempt's stripes, out = the last one's.  two: the attempts run the two-phase coder.
template <class Attempt>
static int encode_attempts(w3_ctx *ctx, Job &J, hipStream_t s, bool two, const uint8_t *d_in, size_t n, size_t block_size, uint32_t nb,
                           uint32_t *d_block_lens, hipEvent_t *evp, uint32_t &cap, Attempt &&attempt) {
    int rc;
    bool cap_raised = false, fault_seen = false;
    uint32_t lds_faults = 0;
    auto read_status = [&](JobStatus &st) -> int {
        HIPCHK(ctx, hipMemcpyAsync(st.w, J.flag.p, sizeof st.w, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        return W3_OK;
    };
    for (int k = 0; k < 4; k++) {
        ENSURE(ctx, J.stripes, (size_t)nb * cap);
        HIPCHK(ctx, hipMemsetAsync(J.flag.p, 0, 4 * ST_WORDS, s));
        if (evp) HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_TOTAL], s));
        if ((rc = attempt(cap))) return rc;
        JobStatus st{};
        if ((rc = read_status(st))) return rc;
        JobAction act = job_classify(st, cap_raised, fault_seen, two);
        if (act == JOB_RECODE) {
            ctx->timing.n_recoded_blocks += st.handed_back();
            rc = twophase_recode(J.tp, s, d_in, n, block_size, nb, (uint8_t *)J.stripes.p, cap, d_block_lens, (uint32_t *)J.flag.p, st.handed_back(), ctx->err);
            if (rc || (rc = read_status(st))) return rc;
            act = job_classify_coded(st, cap_raised);
        }
        if (act == JOB_DONE) break;
        switch (act) {
        case JOB_BALLOT_ROUNDS:   // (w3_jobs.h)
            fault_seen = true;
            lds_faults += st.order_fault();
            use_ballot_rounds(ctx);
            break;
        case JOB_RAISE_CAP:
            cap = worst_stripe_cap(block_size);
            cap_raised = true;
            break;
        case JOB_ERR_ORDER_FAULT: ctx->err = "predict streams differ from their ballot-round re-prediction even without LDS-add rounds (internal error)"; return W3_E_HIP;
        case JOB_ERR_TIMEOUT: ctx->err = "coder pipeline timeout (internal error)"; return W3_E_HIP;
        case JOB_ERR_APM_OOB: ctx->err = "APM kernel: " + std::to_string(st.apm_oob()) + " stores outside the stage's stream and the sink (W3_TUNING store guard)"; return W3_E_HIP;
        default: ctx->err = "stripe overflow at the worst-case bound (internal error)"; return W3_E_HIP;
        }
        ctx->timing.n_recoded_blocks = 0;
    }
    ctx->timing.n_lds_faults = lds_faults;
    return W3_OK;
}

// d_out == nullptr: counting-sink mode (ACStats, helpers.rs:60-90) — the streams are coded into the stripes as usual, the
// pack is skipped and only J.bits (per-block bit counts) is of interest; d_block_lens may then be a scratch buffer.
// Synchronous: returns when the output is complete.  J = the job whose workspace is used (jobs[0] for every synchronous entry point;
// w3_encode_wait redoes a job of its own here).
// d_p != nullptr: no model — the coder runs over the caller's stream d_p (w3_encode_probs_device, which has checked it; `spec` is not read).
static int encode_core(w3_ctx *ctx, Job &J, const w3_model_spec *spec, const uint8_t *d_in, size_t n, size_t block_size,
                       uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens, uint64_t *d_total, void *stream, const uint16_t *d_p = nullptr) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    ParsedSpec ps;
    if (!d_p && (rc = parse_spec(spec, ps))) { ctx->err = "malformed model spec"; return rc; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint32_t nb = (uint32_t)((n + block_size - 1) / block_size);
    memset(&ctx->timing, 0, sizeof ctx->timing);
    ENSURE(ctx, ctx->total, 8);
    uint64_t *total_p = d_total ? d_total : (uint64_t *)ctx->total.p;
    if (nb == 0) {
        HIPCHK(ctx, hipMemsetAsync(total_p, 0, 8, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        return W3_OK;
    }
    if (!d_in || !d_block_lens) return W3_E_INVALID;
    const bool two = d_p || takes_twophase(ctx, ps, block_size, n);   // Counter and slot-state leaves + APM chain (decode: k_generic / k_cm)
    if (ctx->opt_path == W3_PATH_TWOPHASE && !two) { ctx->err = "spec/block size not covered by the two-phase path"; return W3_E_UNSUPPORTED; }
    if (!two && J.index) { ctx->err = "internal: the lane-per-block path runs on job 0"; return W3_E_INVALID; }
    if ((rc = job_prepare(ctx, J, ps, s, two, (ctx->opt.variant & W3_VAR_HALF_CU) != 0, n, block_size, nb))) return rc;

    hipEvent_t *evp = ctx->opt_timing ? J.ev : nullptr;
    uint32_t cap = default_stripe_cap(block_size);
    w3_timing ptm;
    memset(&ptm, 0, sizeof ptm);
    rc = encode_attempts(ctx, J, s, two, d_in, n, block_size, nb, d_block_lens, evp, cap, [&](uint32_t cap_now) -> int {
        int r;
        if (d_p) {   // the coder part of tp_code_stage over the one stream
            memset(&ptm, 0, sizeof ptm);
            TwoPhaseWs &ws = J.tp;
            ws.P_valid = false; ws.used_lds_atomics = false;
            memset(&ws.mix, 0, sizeof ws.mix);
            ws.mix.src[0] = (const uint4 *)d_p; ws.mix.n_src = 1;
            const TpPlan pl = tp_plan(ws, ps);
            r = tp_coder(ws, s, pl.coder, pl.x3, d_in, n, block_size, nb, (uint8_t *)J.stripes.p, cap_now, d_block_lens, (uint32_t *)J.flag.p, evp, &ptm, ctx->err);
            if (r) return r;
            ctx->timing.path = W3_PATH_TWOPHASE;
        } else if (two) {
            memset(&ptm, 0, sizeof ptm);
            r = twophase_encode(J.tp, s, s, ps, d_in, n, block_size, nb, (uint8_t *)J.stripes.p, cap_now, d_block_lens, (uint32_t *)J.flag.p, evp, &ptm, ctx->err);
            if (r) return r;
            ctx->timing.path = W3_PATH_TWOPHASE;
        } else {
            if (evp) HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PREDICT], s));
            LaneIo io;
            io.in = d_in; io.stripe_cap = cap_now; io.out_len = d_block_lens;
            r = lane_run<false>(ctx, s, ps, block_size, n, nb, io);
            if (evp) HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PREDICT + 1], s));
            ctx->timing.path = W3_PATH_GENERIC;
            if (r) return r;
        }
        return W3_OK;
    });
    if (rc) return rc;
    uint64_t total = 0;
    if (d_out) {
        if (evp) HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PACK], s));
        rc = run_pack(ctx, J, s, (const uint8_t *)J.stripes.p, cap, d_block_lens, nb, d_out, out_cap, total_p);
        if (evp) { HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PACK + 1], s)); HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_TOTAL + 1], s)); }
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(&total, total_p, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    } else {
        if (evp) HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_TOTAL + 1], s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    if (d_p) {   // no model: only the coder's, the pack's and the call's events were recorded
        fill_timing(ctx, J, ptm, total, ps, false, d_out != nullptr);
        if (evp) { ctx->timing.coder_ms = elapsed_ev(evp, W3_EV_CODER); ctx->timing.pack_ms = d_out ? elapsed_ev(evp, W3_EV_PACK) : 0.f; ctx->timing.total_ms = elapsed_ev(evp, W3_EV_TOTAL); }
    } else if (two) fill_timing(ctx, J, ptm, total, ps, evp != nullptr, d_out != nullptr);
    else if (evp) { ctx->timing.generic_ms = elapsed_ev(evp, W3_EV_PREDICT); ctx->timing.pack_ms = d_out ? elapsed_ev(evp, W3_EV_PACK) : 0.f; ctx->timing.total_ms = elapsed_ev(evp, W3_EV_TOTAL); }
    ctx->timing.n_parts = 1;
    if (d_out && total > out_cap) { ctx->err = "out_cap too small"; return W3_E_NOSPACE; }
    return W3_OK;
}

extern "C" int w3_encode_blocks_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, size_t block_size,
                                       uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens, uint64_t *d_total, void *stream) {
    if (!ctx) return W3_E_INVALID;
    if (n && !d_out) return W3_E_INVALID;
    int rc = jobs_idle(ctx);
    if (rc) return rc;
    return encode_core(ctx, ctx->jobs[0], spec, d_in, n, block_size, d_out, out_cap, d_block_lens, d_total, stream);
}

// ---------------------------------------------------------------------------
// submit / wait: up to two encodes in flight on one context (main.rs:103-109 run for call k+1's predict phase while call k is
// still being coded).  Each job has its own workspace; the predict phases follow each other on one stream, the APM + coder +
// pack stages on another, so in steady state the chip always holds one call's predict kernels and the previous call's APM
// or coder kernel — in the half-CU shapes (w3_predict.h, w3_coder5.h) that let the two share every CU.
// ---------------------------------------------------------------------------
// twophase_predict_b's choice for the slot-state leaves, as far as the spec and the shape decide it (w3_twophase.h)
static bool slot_sorted_by_default(const ParsedSpec &ps, uint32_t nb, size_t block_size, size_t n) {
    if (nb >= W3_SLOT_SORTED_MAX_BLOCKS || block_size > (1ull << 31)) return false;
    size_t n_slot = 0;
    for (int l = 0; l < ps.n_leaves; l++) {
        if (ps.leaf[l].kind != W3_NODE_SLOT_STATE) continue;
        if (ps.leaf[l].log_cells > 16) return false;
        n_slot++;
    }
    // (two jobs in flight hold two sets of event records, 32 bytes per input byte and leaf: beyond 48 GB a set the call stays synchronous —
    // twophase_predict_b then still picks the replay if the records fit beside everything else, or k_slot)
    return 32ull * n_slot * n <= (48ull << 30);
}

// How submitted calls of this spec and size are kept in flight (w3_jobs.h)
static PipelinePlan pipeline_plan(const ParsedSpec &ps, size_t nb, uint32_t tune) {
    int n_wide = 0;
    for (int l = 0; l < ps.n_leaves; l++) { const int c = leaf_class(ps.leaf[l]); n_wide += c == LEAF_WIDE1 || c == LEAF_WIDE2 || c == LEAF_WAVE; }
    return pipeline_plan(n_wide, ps.n_apm, ps.has_slot, (uint32_t)std::min<size_t>(nb, 0xFFFFFFFFu), tune);
}

// Does w3_encode_submit only enqueue this call (true), or run it to completion inside the call (false: specs outside the predict kernels,
// and specs whose slot-state leaves walk hash maps in HBM)?
static bool submit_pipelines(const w3_ctx *ctx, const ParsedSpec &ps, uint32_t nb, size_t block_size, size_t n) {
    const bool two = nb > 0 && takes_twophase(ctx, ps, block_size, n);
    // Specs with slot-state leaves are pipelined when the leaves run as the sorted replay (w3_slot2.h: no hash maps sized from the memory
    // that happens to be free) — two jobs at most: a job's event records are 32 bytes per input byte and leaf.
    const bool slot_async = ps.has_slot && slot_sorted_by_default(ps, nb, block_size, n) && !(ctx->opt.variant & (W3_VAR_SLOT_TABLE | W3_VAR_NO_LDS_ATOMICS)) && ctx->lds_order != 0;
    return two && !(ps.has_slot && !slot_async);
}

static int ensure_pipeline(w3_ctx *ctx) {
    // The two stages must not share a hardware queue (HIP maps streams onto GPU_MAX_HW_QUEUES = 4 queues per priority level by
    // default, round-robin: two streams of one level can land on the same queue and then run one after the other).  Streams of
    // different PRIORITY levels use different queues: the code stage — it carries the latency chain — gets the high level.
    if (!ctx->s_pred || !ctx->s_code[W3_MAX_JOBS - 1]) {
        int lo_p = 0, hi_p = 0;
        HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&lo_p, &hi_p));
        const bool pred_high = (ctx->opt.tune & 1u) != 0;   // W3_OPT_TUNE bit 0
        const bool plain = !(ctx->opt.tune & (1u | 16u));   // (tuning variants create their own)
        if (!ctx->s_pred && plain) ctx->s_pred = stream_pool().take(ctx->device * 8L);
        if (!ctx->s_pred) HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->s_pred, hipStreamNonBlocking, pred_high ? hi_p : 0));
        // (created one after the other on one level: HIP deals that level's hardware queues out round-robin, so the W3_MAX_JOBS = 4 code
        // streams get a queue each and the free-running jobs' coders really run side by side)
        for (auto &sc : ctx->s_code) {
            if (!sc && plain) sc = stream_pool().take(ctx->device * 8L + 1);
            if (!sc) HIPCHK(ctx, hipStreamCreateWithPriority(&sc, hipStreamNonBlocking, (pred_high || (ctx->opt.tune & 16u)) ? 0 : hi_p));
        }
        ctx->pooled_streams = plain;
    }
    for (auto &J : ctx->jobs) {
        for (hipEvent_t *e : {&J.ev_done, &J.ev_in, &J.ev_a, &J.ev_apm})
            if (!*e) HIPCHK(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
        if (!J.h_status) HIPCHK(ctx, hipHostMalloc((void **)&J.h_status, 32, hipHostMallocDefault));
        for (auto &e : J.ev)
            if (!e) HIPCHK(ctx, hipEventCreate(&e));
    }
    return W3_OK;
}

// APM stages + coder + pack + status read-back of an enqueued job, on the code stream
static int enqueue_code(w3_ctx *ctx, Job &J, hipEvent_t wait_ev, hipEvent_t rec_after_apm) {
    const KeptCall &c = J.call;
    hipStream_t sp = ctx->s_pred, sc = J.sc;
    hipEvent_t *evp = J.timed ? J.ev : nullptr;
    int rc = tp_code_stage(J.tp, sp, sc, c.ps, c.d_in, c.n, c.block_size, J.nb, (uint8_t *)J.stripes.p, J.cap, J.d_block_lens, (uint32_t *)J.flag.p,
                           wait_ev, rec_after_apm, evp, &J.tm, ctx->err);
    if (rc) return rc;
    if (evp) HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PACK], sc));
    rc = run_pack(ctx, J, sc, (const uint8_t *)J.stripes.p, J.cap, J.d_block_lens, J.nb, J.d_out, J.out_cap, J.d_total);
    if (evp) { HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PACK + 1], sc)); HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_TOTAL + 1], sc)); }
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(J.h_status, J.flag.p, 4 * ST_WORDS, hipMemcpyDeviceToHost, sc));
    HIPCHK(ctx, hipMemcpyAsync(J.h_status + ST_WORDS, J.d_total, 8, hipMemcpyDeviceToHost, sc));
    HIPCHK(ctx, hipEventRecord(J.ev_done, sc));
    J.code_pending = false;
    return W3_OK;
}

extern "C" int w3_encode_submit(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, size_t block_size,
                                uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens, uint64_t *d_total, void *stream, int *job) {
    if (!ctx || !job) return W3_E_INVALID;
    *job = -1;
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    if (n && (!d_out || !d_in || !d_block_lens)) return W3_E_INVALID;
    if (!d_total) { ctx->err = "w3_encode_submit needs d_total"; return W3_E_INVALID; }
    ParsedSpec ps;
    if ((rc = parse_spec(spec, ps))) { ctx->err = "malformed model spec"; return rc; }
    const uint32_t nb = (uint32_t)((n + block_size - 1) / block_size);
    const PipelinePlan plan = pipeline_plan(ps, nb, ctx->opt.tune);
    int busy[W3_MAX_JOBS];
    for (int k = 0; k < W3_MAX_JOBS; k++) busy[k] = ctx->jobs[k].state;
    const SlotPick pick = pick_slot(busy, W3_MAX_JOBS, ctx->next_job, plan.depth);
    if (pick.slot < 0) {
        ctx->err = std::to_string(pick.in_flight) + " jobs are in flight already (at most " + std::to_string(plan.depth) + " for an input of this size): w3_encode_wait the oldest one first";
        return W3_E_INVALID;
    }
    const int j = pick.slot;
    Job &J = ctx->jobs[j];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!submit_pipelines(ctx, ps, nb, block_size, n)) {
        // Not pipelined: the lane-per-block kernels (any spec the predict kernels do not cover) and specs whose slot-state leaves walk
        // hash maps in HBM (k_slot: sized from the memory that is free at the time) run to completion here, on job 0's workspace.
        for (auto &O : ctx->jobs) {   // let the other jobs' kernels finish first; their status is in pinned memory already
            if (O.state != 1) continue;
            if (O.code_pending && (rc = enqueue_code(ctx, O, nullptr, nullptr))) return rc;
            HIPCHK(ctx, hipEventSynchronize(O.ev_done));
            if (O.index == 0 && O.timed && !O.tm_snap) {   // job 0's events are about to be recorded again
                memset(&O.tm_ev, 0, sizeof O.tm_ev);
                collect_timing(O.ev, O.tp, O.call.ps.n_apm > 0, O.call.ps.has_slot, O.call.ps.has_mix, true, O.tm_ev);
                O.tm_snap = true;
            }
        }
        // Completed by w3_encode_wait like any other job: THAT call returns what the synchronous call returned (W3_E_NOSPACE with
        // d_total = the need included), so a caller that follows the submit / wait contract sees one behaviour for every spec.
        const w3_timing keep = ctx->timing;
        J.sync_rc = encode_core(ctx, ctx->jobs[0], spec, d_in, n, block_size, d_out, out_cap, d_block_lens, d_total, stream);
        J.state = 2; J.tm = ctx->timing;
        ctx->timing = keep;
        *job = j; ctx->next_job = j + 1; ctx->last_job = j;
        return W3_OK;
    }
    if ((rc = ensure_pipeline(ctx))) return rc;
    J.call.keep(spec, ps, d_in, n, block_size);
    J.d_out = d_out; J.out_cap = out_cap; J.d_block_lens = d_block_lens; J.d_total = d_total;
    J.timed = ctx->opt_timing != 0; J.tm_snap = false;
    J.nb = nb;
    J.sc = plan.free_run ? ctx->s_code[j] : ctx->s_code[0];
    memset(&J.tm, 0, sizeof J.tm);
    hipStream_t sp = ctx->s_pred;
    // after whatever produced d_in on the caller's stream
    hipStream_t s_in = stream ? (hipStream_t)stream : ctx->stream;
    HIPCHK(ctx, hipEventRecord(J.ev_in, s_in));
    HIPCHK(ctx, hipStreamWaitEvent(sp, J.ev_in, 0));
    if ((rc = job_prepare(ctx, J, J.call.ps, sp, true, !(ctx->opt.variant & W3_VAR_FULL_CU), n, block_size, nb))) return rc;
    J.call.vcall = J.tp.verify_calls;
    J.cap = default_stripe_cap(block_size);
    ENSURE(ctx, J.stripes, (size_t)nb * J.cap);
    hipEvent_t *evp = J.timed ? J.ev : nullptr;
    HIPCHK(ctx, hipMemsetAsync(J.flag.p, 0, 4 * ST_WORDS, sp));
    if (evp) HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_TOTAL], sp));
    // The order in which the two jobs' kernels reach the chip (measured, profiles/r3_pipeline/: kernels that fill the LDS — the
    // partition passes, the time-ordered leaves, k_apm0 — only slow each other down when they share CUs; the rank kernels, bound
    // by their scattered stores, and the coder, one latency chain per lane, run well side by side):
    //     first predict half of THIS job  ->  APM stages of the OTHER job  ->  coder of the other job  BESIDE  rank kernels of this job
    // So the other job's code stage is enqueued here, between this job's two predict halves (W3_OPT_TUNE bit 2: no such order).
    // Free-running jobs (small inputs) need no such order: the chip is mostly idle while a call is coded, so every job's code stage
    // goes to its own stream at once and the coders of up to W3_MAX_JOBS calls run side by side (each a latency chain on a few CUs).
    const bool ordered = !(ctx->opt.tune & 4u) && !plan.free_run;
    Job *prev = ctx->last_job >= 0 && ctx->last_job != j ? &ctx->jobs[ctx->last_job] : nullptr;
    if (prev && !(prev->state == 1 && prev->code_pending)) prev = nullptr;
    if (prev && !ordered && (rc = enqueue_code(ctx, *prev, nullptr, nullptr))) return rc;   // (an ordered job before a free-running one: its code stage goes out now)
    const ParsedSpec &kps = J.call.ps;
    rc = twophase_predict_a(J.tp, sp, kps, d_in, n, block_size, nb, evp, ctx->err, ordered);
    if (!rc && ordered) {
        HIPCHK(ctx, hipEventRecord(J.ev_a, sp));
        if (prev) {
            rc = enqueue_code(ctx, *prev, J.ev_a, prev->ev_apm);
            if (!rc) HIPCHK(ctx, hipStreamWaitEvent(sp, prev->ev_apm, 0));
        }
    }
    if (!rc) rc = twophase_predict_b(J.tp, sp, kps, d_in, n, block_size, nb, tp_plan(J.tp, kps).need_P, nullptr, evp, &J.tm, ctx->err);
    if (!rc) rc = tp_after_predict(J.tp, sp, kps, d_in, n, block_size, nb, (uint32_t *)J.flag.p, ctx->err);
    if (!rc) {
        J.state = 1; J.code_pending = true;
        if (!ordered) rc = enqueue_code(ctx, J, nullptr, nullptr);
    }
    if (rc) {   // leave nothing of either job running behind an error return
        (void)hipDeviceSynchronize();
        J.state = 0; J.code_pending = false;
        return rc;
    }
    *job = j; ctx->next_job = j + 1; ctx->last_job = j;
    return W3_OK;
}

extern "C" int w3_encode_max_in_flight(const w3_model_spec *spec, size_t n, size_t block_size) {
    if (!block_size) return 0;
    const size_t nb = (n + block_size - 1) / block_size;
    ParsedSpec ps;   // (no spec: a model with wide leaves and an APM stage, the most conservative answer)
    if (spec) { if (parse_spec(spec, ps)) return 0; }
    else { ps.n_leaves = 1; ps.leaf[0] = w3_node{}; ps.leaf[0].kind = W3_NODE_ORDERN; ps.leaf[0].bits = 19; ps.leaf[0].align = 3; ps.n_apm = 1; }
    return pipeline_plan(ps, nb, 0u).depth;
}

extern "C" int w3_encode_wait(w3_ctx *ctx, int job) {
    if (!ctx || job < 0 || job >= W3_MAX_JOBS) return W3_E_INVALID;
    Job &J = ctx->jobs[job];
    if (J.state == 0) { ctx->err = "no such job in flight"; return W3_E_INVALID; }
    J.total_valid = false;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (J.state == 2) { J.state = 0; ctx->timing = J.tm; return J.sync_rc; }
    if (J.code_pending) {   // no later submit has placed this job's code stage: it goes out now
        const int rc = enqueue_code(ctx, J, nullptr, nullptr);
        if (rc) { (void)hipDeviceSynchronize(); J.state = 0; J.code_pending = false; return rc; }
    }
    HIPCHK(ctx, hipEventSynchronize(J.ev_done));
    J.state = 0;
    JobStatus st;
    uint64_t total;
    memcpy(st.w, J.h_status, sizeof st.w);
    memcpy(&total, J.h_status + ST_WORDS, 8);
    const KeptCall &c = J.call;
    switch (const JobAction act = job_classify_waited(st)) {
    case JOB_DONE: break;
    case JOB_ERR_TIMEOUT: ctx->err = "coder pipeline timeout (internal error)"; return W3_E_HIP;
    case JOB_ERR_APM_OOB: ctx->err = "APM kernel: stores outside the stage's stream and the sink (W3_TUNING store guard)"; return W3_E_HIP;
    default: {
        // Rare: a stripe overflowed the 2N+64 bound, the fast coder handed blocks back, or the sampled verification saw the LDS-add
        // rounds misbehave.  Let the other job's kernels finish (its output is complete then, its status in pinned memory) and
        // run this call again synchronously on this job's workspace: encode_core's own retry loop deals with each case.
        HIPCHK(ctx, hipDeviceSynchronize());
        if (act == JOB_BALLOT_ROUNDS) use_ballot_rounds(ctx);
        VcallPin pin(ctx, c.vcall);   // (the same call: the same rotation)
        const int rc = encode_core(ctx, J, &c.spec, c.d_in, c.n, c.block_size, J.d_out, J.out_cap, J.d_block_lens, J.d_total, ctx->stream);
        ctx->timing.n_lds_faults += st.order_fault();
        return rc;
    }
    }
    J.total_out = total; J.total_valid = true;
    memset(&ctx->timing, 0, sizeof ctx->timing);
    if (J.timed && J.tm_snap) ctx->timing = J.tm_ev;   // (the event times; everything else in it is zero)
    fill_timing(ctx, J, J.tm, total, c.ps, J.timed && !J.tm_snap, true);
    if (total > J.out_cap) { ctx->err = "out_cap too small"; return W3_E_NOSPACE; }
    return W3_OK;
}

// ---------------------------------------------------------------------------
// Host buffers, asynchronous (ABI v8): compress() of main.rs:89-113 reads a file and writes a file, so what a host sees is
// PCIe in, encode, PCIe out.  A call here is those three as a pipeline ACROSS calls: the input of call k+1 travels while call k
// is encoded (w3_encode_submit: up to four encodes in flight) and the streams of call k-1 travel back.  Copies run on two
// streams of their own (one per direction: the link is full duplex); from pinned host memory they are asynchronous, from
// pageable memory HIP stages them and the enqueueing call blocks — the encodes already submitted keep the GPU busy meanwhile.
// ---------------------------------------------------------------------------
static int host_streams(w3_ctx *ctx) {
    // The copies of BOTH directions go to the context's own stream — idle while calls are pipelined (only the synchronous entry points
    // launch on it) — in the order the host needs them: a call's input long before its encode is submitted, a call's streams after it
    // has been waited for; together 24 ms of a 68 ms step at 1e9 B, so the link need not run full duplex.  NO stream is created: HIP maps
    // streams onto 4 hardware queues per priority level (unless GPU_MAX_HW_QUEUES says otherwise) by the queues' use at creation, and a
    // copy stream that lands on the predict stream's queue holds that call's kernels back for the length of a copy (measured: 84.5 ms
    // per call with two copy streams of their own against 72.6 with 8 hardware queues in the environment, profiles/r4_host_path/).
    // W3_OPT_TUNE bit 16: two copy streams of their own, one per direction (for hosts that do raise GPU_MAX_HW_QUEUES).
    if (ctx->opt.tune & 65536u) {
        if (!ctx->s_h2d_own) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->s_h2d_own, hipStreamNonBlocking));
        if (!ctx->s_d2h_own) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->s_d2h_own, hipStreamNonBlocking));
        ctx->s_h2d = ctx->s_h2d_own; ctx->s_d2h = ctx->s_d2h_own;
    } else {
        ctx->s_h2d = ctx->s_d2h = ctx->stream;
    }
    for (auto &h : ctx->hj)
        if (!h.ev_d2h) HIPCHK(ctx, hipEventCreateWithFlags(&h.ev_d2h, hipEventDisableTiming));
    return W3_OK;
}

static int host_depth(const w3_model_spec *spec, size_t n, size_t block_size) {
    return std::min(W3_MAX_HOST_JOBS, w3_encode_max_in_flight(spec, n, block_size) + 1);
}

// Submit the encodes of host jobs whose input is on its way, oldest first, while device job slots are free.
static void host_start_pending(w3_ctx *ctx) {
    for (;;) {
        HostJob *h = nullptr;
        for (auto &x : ctx->hj)
            if (x.state == 1 && (!h || x.seq < h->seq)) h = &x;
        if (!h) return;
        const KeptCall &c = h->call;
        int in_flight = 0;
        for (const auto &o : ctx->jobs) in_flight += o.state != 0;
        if (in_flight >= pipeline_plan(c.ps, h->nb, 0u).depth) return;
        // (the job starts behind everything enqueued on the H2D stream so far: its own input was the last of it)
        VcallPin pin(ctx, c.vcall);
        h->rc = w3_encode_submit(ctx, &c.spec, c.d_in, c.n, c.block_size, (uint8_t *)h->d_out.p, h->dcap,
                                 (uint32_t *)h->d_lens.p, (uint64_t *)h->d_total.p, ctx->s_h2d, &h->djob);
        h->state = h->rc ? 3 : 2;   // (a refused submit is reported by the wait)
    }
}

// A call whose output went beyond the realistic bound its device buffer was sized for (adversarial input: up to 16 n) is encoded once
// more, alone, with the room it asked for: into `out`, grown to `need` bytes.  djob: the slot w3_encode_submit gave it.
static int redo_with_room(w3_ctx *ctx, const KeptCall &c, int djob, uint64_t vcall, DevBuf &out, size_t &cap, uint64_t need, DevBuf &lens, DevBuf &total) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());   // (the other jobs' kernels: their outputs are complete afterwards, their status words in pinned memory)
    ENSURE(ctx, out, (size_t)need);
    cap = (size_t)need;
    const uint32_t nb = (uint32_t)((c.n + c.block_size - 1) / c.block_size);
    Job &J = ctx->jobs[submit_pipelines(ctx, c.ps, nb, c.block_size, c.n) ? djob : 0];   // (what w3_encode_submit ran synchronously ran on job 0)
    VcallPin pin(ctx, vcall);
    return encode_core(ctx, J, &c.spec, c.d_in, c.n, c.block_size, (uint8_t *)out.p, cap, (uint32_t *)lens.p, (uint64_t *)total.p, ctx->stream);
}

// state 2 -> 3: wait for the job's encode; rc and the compressed size are known afterwards
static void host_finish_device(w3_ctx *ctx, HostJob &h) {
    h.rc = w3_encode_wait(ctx, h.djob);
    h.tm = ctx->timing;
    h.total = 0;
    h.state = 3;
    auto read_total = [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(&h.total, h.d_total.p, 8, hipMemcpyDeviceToHost, ctx->s_d2h));
        HIPCHK(ctx, hipStreamSynchronize(ctx->s_d2h));
        return W3_OK;
    };
    if (h.rc == W3_OK || h.rc == W3_E_NOSPACE) {
        const Job &ds = ctx->jobs[h.djob];
        if (ds.total_valid) h.total = ds.total_out;   // (the usual case: no device access, no wait for a copy that is in flight on the copy stream)
        else { const int r = read_total(); if (r) h.rc = r; }
    }
    if (h.rc == W3_E_NOSPACE && h.total > h.dcap) {   // (the device buffer is sized for 2 n + 64 per block, the stripes' own bound)
        h.rc = redo_with_room(ctx, h.call, h.djob, h.call.vcall, h.d_out, h.dcap, h.total, h.d_lens, h.d_total);
        if (!h.rc) h.rc = read_total();
    }
}

// vcall: the call's number for the verification's rotation (w3_encode_blocks: its own, for every piece), or -1: a new one
static int host_submit_core(w3_ctx *ctx, const w3_model_spec *spec, const ParsedSpec &ps, const uint8_t *in, size_t n, size_t block_size,
                            uint8_t *out, size_t out_cap, uint32_t *block_lens, int *hjob, int64_t vcall = -1) {
    int rc = host_streams(ctx);
    if (rc) return rc;
    const size_t nb = (n + block_size - 1) / block_size;
    int busy[W3_MAX_HOST_JOBS];
    for (int k = 0; k < W3_MAX_HOST_JOBS; k++) busy[k] = ctx->hj[k].state;
    const int depth = host_depth(spec, n, block_size);
    const SlotPick pick = pick_slot(busy, W3_MAX_HOST_JOBS, 0, depth);   // (the first free slot)
    const int slot = pick.slot;
    if (slot < 0) {
        ctx->err = std::to_string(pick.in_flight) + " host-buffer jobs are in flight already (at most " + std::to_string(depth) + " for an input of this size): w3_encode_host_wait the oldest one first";
        return W3_E_INVALID;
    }
    HostJob &h = ctx->hj[slot];
    h.nb = nb; h.out = out; h.out_cap = out_cap; h.block_lens = block_lens;
    h.djob = -1; h.rc = W3_OK; h.total = 0;
    memset(&h.tm, 0, sizeof h.tm);
    // the device output buffer: the realistic bound, never more than the hard one (a call beyond it is redone: host_finish_device)
    h.dcap = std::min<size_t>(w3_max_compressed_size(n, block_size), 2 * n + 64 * nb + 64);
    ENSURE(ctx, h.d_in, std::max<size_t>(n, 16));
    ENSURE(ctx, h.d_out, std::max<size_t>(h.dcap, 16));
    ENSURE(ctx, h.d_lens, std::max<size_t>(nb * 4, 16));
    ENSURE(ctx, h.d_total, 8);
    h.call.keep(spec, ps, (const uint8_t *)h.d_in.p, n, block_size);
    h.call.vcall = vcall >= 0 ? (uint64_t)vcall : verify_call(ctx, n, block_size);
    HIPCHK(ctx, hipMemcpyAsync(h.d_in.p, in, n, hipMemcpyHostToDevice, ctx->s_h2d));
    h.seq = ++ctx->hseq;
    h.state = 1;
    host_start_pending(ctx);
    *hjob = slot;
    return W3_OK;
}

// out / out_cap: where the streams go (w3_encode_blocks binds a chunk's destination only now: it is the sum of the earlier chunks'
// sizes).  *out_len is set even on W3_E_NOSPACE; the length table is copied in either case.
static int host_wait_core(w3_ctx *ctx, int hjob, uint8_t *out, size_t out_cap, size_t *out_len) {
    HostJob &h = ctx->hj[hjob];
    // jobs are encoded in the order they were submitted: whatever is older goes through the device first
    while (h.state == 1 || h.state == 2) {
        HostJob *o = nullptr;
        for (auto &x : ctx->hj)
            if (x.state == 2 && (!o || x.seq < o->seq)) o = &x;
        if (o) host_finish_device(ctx, *o);
        const int before = h.state;
        host_start_pending(ctx);   // FIRST: the next call's kernels reach the GPU before this call's streams start travelling back
        if (!o && h.state == before) { h.state = 0; ctx->err = "host-buffer job could not be submitted (internal error)"; return W3_E_HIP; }
    }
    int rc = h.rc;
    *out_len = (size_t)h.total;
    if (rc == W3_OK || rc == W3_E_NOSPACE) {
        auto fetch = [&]() -> int {
            if (h.nb && h.block_lens) HIPCHK(ctx, hipMemcpyAsync(h.block_lens, h.d_lens.p, h.nb * 4, hipMemcpyDeviceToHost, ctx->s_d2h));
            const bool fits = rc == W3_OK && h.total <= out_cap && (out || !h.total);
            if (fits && h.total) HIPCHK(ctx, hipMemcpyAsync(out, h.d_out.p, (size_t)h.total, hipMemcpyDeviceToHost, ctx->s_d2h));
            HIPCHK(ctx, hipEventRecord(h.ev_d2h, ctx->s_d2h));
            HIPCHK(ctx, hipEventSynchronize(h.ev_d2h));
            if (!fits) { if (rc == W3_OK) ctx->err = "out_cap too small"; return W3_E_NOSPACE; }
            return W3_OK;
        };
        rc = fetch();
    }
    ctx->timing = h.tm;
    h.state = 0;
    return rc;
}

extern "C" int w3_encode_host_max_in_flight(const w3_model_spec *spec, size_t n, size_t block_size) {
    if (!block_size || (spec && w3_spec_validate(spec))) return 0;
    return host_depth(spec, n, block_size);
}

extern "C" int w3_encode_host_submit(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, size_t block_size,
                                     uint8_t *out, size_t out_cap, uint32_t *block_lens, int *hjob) {
    if (!ctx || !hjob) return W3_E_INVALID;
    *hjob = -1;
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    ParsedSpec ps;
    if ((rc = parse_spec(spec, ps))) { ctx->err = "malformed model spec"; return rc; }
    if (n == 0 || !in || !block_lens) { ctx->err = "w3_encode_host_submit needs input and a length table"; return W3_E_INVALID; }
    for (const auto &J : ctx->jobs)   // (the two levels are not mixed: the host jobs count the device job slots as theirs)
        if (J.state != 0) {
            bool ours = false;
            for (const auto &h : ctx->hj) ours |= h.state == 2 && h.djob == J.index;
            if (!ours) { ctx->err = "w3_encode_submit jobs are in flight on this context: w3_encode_wait them first"; return W3_E_INVALID; }
        }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return host_submit_core(ctx, spec, ps, in, n, block_size, out, out_cap, block_lens, hjob);
}

extern "C" int w3_encode_host_wait(w3_ctx *ctx, int hjob, size_t *out_len) {
    if (!ctx || !out_len || hjob < 0 || hjob >= W3_MAX_HOST_JOBS) return W3_E_INVALID;
    *out_len = 0;
    if (ctx->hj[hjob].state == 0) { ctx->err = "no such host-buffer job in flight"; return W3_E_INVALID; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return host_wait_core(ctx, hjob, ctx->hj[hjob].out, ctx->hj[hjob].out_cap, out_len);
}

// ---------------------------------------------------------------------------
// ACStats (helpers.rs:60-90): the counting sink every published figure of the reference comes from
// ---------------------------------------------------------------------------
extern "C" int w3_encode_stats_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, size_t block_size,
                                      uint32_t *d_block_bits, void *stream) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    const size_t nb = (n + block_size - 1) / block_size;
    if (nb == 0) return w3_spec_validate(spec);
    if (!d_in || !d_block_bits) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = jobs_idle(ctx))) return rc;
    ENSURE(ctx, ctx->lens, nb * 4);
    rc = encode_core(ctx, ctx->jobs[0], spec, d_in, n, block_size, nullptr, 0, (uint32_t *)ctx->lens.p, nullptr, stream);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(d_block_bits, ctx->jobs[0].bits.p, nb * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return W3_OK;
}

// ---------------------------------------------------------------------------
// code from a caller's probability stream (include/w3hip.h: w3_encode_probs_device)
// ---------------------------------------------------------------------------
// Everything before the coder: the arguments, and the zero count of d_p.  The coders rely on p in 1 .. 65535, so NO coder kernel is
// launched unless the count read back here is 0.
static int probs_check(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, const uint16_t *d_p, hipStream_t s) {
    if (!d_in || !d_p) return W3_E_INVALID;
    if (((uintptr_t)d_p & 15u) != 0) { ctx->err = "d_p must be 16-byte aligned"; return W3_E_INVALID; }
    if (block_size > (1u << 24) || n < 8) { ctx->err = "a caller's stream is coded by the two-phase coders: n >= 8, block_size <= 2^24"; return W3_E_UNSUPPORTED; }
    ENSURE(ctx, ctx->probs_res, 16);
    const unsigned long long init[2] = {0ull, ~0ull};
    unsigned long long res[2] = {0ull, ~0ull};
    HIPCHK(ctx, hipMemcpyAsync(ctx->probs_res.p, init, 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_count_zero_p, dim3((unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, 256 * 8)), dim3(256), 0, s, (const uint4 *)d_p, (uint64_t)n,
                       (unsigned long long *)ctx->probs_res.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(res, ctx->probs_res.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (res[0]) {
        ctx->err = "d_p holds " + std::to_string(res[0]) + " zero probabilities, the first at step " + std::to_string(res[1]) + " (the coder needs p in 1 .. 65535)";
        return W3_E_INVALID;
    }
    return W3_OK;
}

extern "C" int w3_encode_probs_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, const uint16_t *d_p,
                                      uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens, uint64_t *d_total, void *stream) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    if (n && (!d_out || !d_block_lens)) return W3_E_INVALID;
    if ((rc = jobs_idle(ctx))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (n == 0) {   // (no blocks: a total of 0, as w3_encode_blocks_device gives)
        ENSURE(ctx, ctx->total, 8);
        HIPCHK(ctx, hipMemsetAsync(d_total ? (void *)d_total : ctx->total.p, 0, 8, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        return W3_OK;
    }
    if ((rc = probs_check(ctx, d_in, n, block_size, d_p, s))) return rc;
    return encode_core(ctx, ctx->jobs[0], nullptr, d_in, n, block_size, d_out, out_cap, d_block_lens, d_total, stream, d_p);
}

extern "C" int w3_encode_stats_probs_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, const uint16_t *d_p,
                                            uint32_t *d_block_bits, void *stream) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    const size_t nb = (n + block_size - 1) / block_size;
    if (nb == 0) return W3_OK;
    if (!d_block_bits) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = jobs_idle(ctx))) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = probs_check(ctx, d_in, n, block_size, d_p, s))) return rc;
    ENSURE(ctx, ctx->lens, nb * 4);
    if ((rc = encode_core(ctx, ctx->jobs[0], nullptr, d_in, n, block_size, nullptr, 0, (uint32_t *)ctx->lens.p, nullptr, stream, d_p))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_block_bits, ctx->jobs[0].bits.p, nb * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return W3_OK;
}

extern "C" int w3_encode_stats(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, size_t block_size, uint32_t *block_bits) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    const size_t nb = (n + block_size - 1) / block_size;
    if (nb == 0) return w3_spec_validate(spec);
    if (!in || !block_bits) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = jobs_idle(ctx))) return rc;
    ENSURE(ctx, ctx->io_in, n);
    ENSURE(ctx, ctx->lens, nb * 4);
    HIPCHK(ctx, hipMemcpyAsync(ctx->io_in.p, in, n, hipMemcpyHostToDevice, ctx->stream));
    rc = encode_core(ctx, ctx->jobs[0], spec, (const uint8_t *)ctx->io_in.p, n, block_size, nullptr, 0, (uint32_t *)ctx->lens.p, nullptr, ctx->stream);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(block_bits, ctx->jobs[0].bits.p, nb * 4, hipMemcpyDeviceToHost));
    return W3_OK;
}

extern "C" int w3_decode_blocks_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t in_len, const uint32_t *d_block_lens,
                                       size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *d_out, void *stream) {
    int rc = check_args(ctx, (size_t)orig_len, block_size);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;   // (job 0's HuffHistory tables, length scan and model tables)
    ParsedSpec ps;
    if ((rc = parse_spec(spec, ps))) { ctx->err = "malformed model spec"; return rc; }
    const uint64_t nb = (orig_len + block_size - 1) / block_size;
    if (nb != nblocks) { ctx->err = "nblocks does not match orig_len/block_size"; return W3_E_INVALID; }
    if (nb == 0) return W3_OK;
    if (!d_in || !d_block_lens || !d_out) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = stage_huff(ctx, s, ps))) return rc;
    if ((rc = check_len_table(ctx, s, d_block_lens, (uint32_t)nb, in_len))) return rc;
    LaneIo io;
    io.cin = d_in; io.clens = d_block_lens; io.dout = d_out;
    rc = lane_run<true>(ctx, s, ps, block_size, orig_len, (uint32_t)nb, io);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    return W3_OK;
}


// ---------------------------------------------------------------------------
// CRC-32 per block (w3_crc.h)
// ---------------------------------------------------------------------------
static_assert(sizeof(CrcSeg) == 16, "w3_crc.h segment layout");
#define W3_CRC_WS_SLICES 256u   // byte offset of the slices' CRCs in ctx->crc_ws (the result words sit in front of them)

// Enqueue the CRCs of nseg segments of d_base on s: uniform blocks of block_size over n bytes (d_segs == nullptr), or the explicit list
// d_segs (none longer than max_len).  d_out != nullptr: d_out[k] = segment k's CRC.  check: every CRC is compared with d_want[k]
// (implicit form) or d_segs[k].want, and the result words ctx->crc_ws[0 .. 16) = {lowest mismatching segment or ~0, mismatches} are
// written (crc_fetch brings them to ctx->crc_res).  Does not synchronise.
static int crc_enqueue(w3_ctx *ctx, hipStream_t s, const uint8_t *d_base, uint64_t n, uint32_t block_size, const CrcSeg *d_segs, uint64_t nseg,
                       uint32_t max_len, uint32_t *d_out, const uint32_t *d_want, bool check) {
    if (nseg == 0 && !check) return W3_OK;
    const uint32_t spb = std::max(1u, crc_slices_of(max_len));
    const uint64_t nsl = nseg * spb;
    const bool direct = spb == 1 && !check && d_out;   // one slice per segment and nothing to compare: the slices' CRCs are the answer
    ENSURE(ctx, ctx->crc_ws, W3_CRC_WS_SLICES + (direct ? 0 : (size_t)nsl * 4));
    uint8_t *ws = (uint8_t *)ctx->crc_ws.p;
    if (check) {
        HIPCHK(ctx, hipMemsetAsync(ws, 0xFF, 8, s));
        HIPCHK(ctx, hipMemsetAsync(ws + 8, 0, 8, s));
    }
    if (nseg == 0) return W3_OK;
    uint32_t *d_slices = direct ? d_out : (uint32_t *)(ws + W3_CRC_WS_SLICES);
    hipLaunchKernelGGL(k_crc32_slices, dim3((uint32_t)std::min<uint64_t>((nsl + 3) / 4, 2048)), dim3(256), 0, s, d_base, n, block_size, d_segs, nseg, spb,
                       d_slices);
    HIPCHK(ctx, hipGetLastError());
    if (direct) return W3_OK;
    hipLaunchKernelGGL(k_crc32_fold, dim3((uint32_t)std::min<uint64_t>((nseg + 255) / 256, 1024)), dim3(256), 0, s, n, block_size, d_segs, nseg, spb,
                       (const uint32_t *)d_slices, d_out, d_want, check ? 1 : 0, (unsigned long long *)ws);
    HIPCHK(ctx, hipGetLastError());
    return W3_OK;
}
// the verify's 16 result bytes, on their way to ctx->crc_res behind the kernels (valid once s has been synchronised)
static int crc_fetch(w3_ctx *ctx, hipStream_t s) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->crc_res, ctx->crc_ws.p, 16, hipMemcpyDeviceToHost, s));
    return W3_OK;
}

// What a checked call reports (include/w3hip.h): the lowest bad block and the count, accumulated over the device calls it is made of.
struct CrcReport {
    uint64_t bad = ~0ull, n_bad = 0;
    void add(uint64_t block, uint64_t count) { if (count) { bad = std::min(bad, block); n_bad += count; } }
    int finish(w3_ctx *ctx, w3_check *chk) const {
        chk->bad_block = bad; chk->n_bad = n_bad;
        if (!n_bad) return W3_OK;
        ctx->err = "block " + std::to_string(bad) + " does not match its CRC-32 (" + std::to_string(n_bad) + " of the verified blocks do not)";
        return W3_E_CORRUPT;
    }
};
// a checked call's w3_check argument: W3_E_INVALID without a table; the outputs start as "nothing found"
static int check_arg(w3_ctx *ctx, w3_check *chk) {
    if (!chk || !chk->crc) { if (ctx) ctx->err = "a checked call needs a w3_check with its CRC table"; return W3_E_INVALID; }
    chk->bad_block = ~0ull; chk->n_bad = 0;
    return W3_OK;
}

extern "C" int w3_crc32_blocks_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, uint32_t *d_crc, void *stream) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;   // (the slices' workspace is the context's)
    if (n == 0) return W3_OK;
    if (!d_in || !d_crc) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint64_t nb = (n + block_size - 1) / block_size;
    if ((rc = crc_enqueue(ctx, s, d_in, n, (uint32_t)block_size, nullptr, nb, (uint32_t)std::min<uint64_t>(block_size, n), d_crc, nullptr, false))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    return W3_OK;
}

extern "C" int w3_crc32_verify_device(w3_ctx *ctx, const uint8_t *d_data, size_t n, size_t block_size, const uint32_t *d_crc, uint64_t *bad_block,
                                      uint64_t *n_bad, void *stream) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;
    if (bad_block) *bad_block = ~0ull;
    if (n_bad) *n_bad = 0;
    if (n == 0) return W3_OK;
    if (!d_data || !d_crc) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint64_t nb = (n + block_size - 1) / block_size;
    if ((rc = crc_enqueue(ctx, s, d_data, n, (uint32_t)block_size, nullptr, nb, (uint32_t)std::min<uint64_t>(block_size, n), nullptr, d_crc, true))) return rc;
    if ((rc = crc_fetch(ctx, s))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    CrcReport rep;
    rep.add(ctx->crc_res[0], ctx->crc_res[1]);
    w3_check out{d_crc, 0, 0};
    rc = rep.finish(ctx, &out);
    if (bad_block) *bad_block = out.bad_block;
    if (n_bad) *n_bad = out.n_bad;
    return rc;
}

// ---------------------------------------------------------------------------
// host-buffer entry points
// ---------------------------------------------------------------------------
// How a host-buffer call is cut into pipelined pieces (whole blocks each).  The pieces are calls of w3_encode_host_submit, so piece
// k+1's input travels while piece k is encoded and piece k-1's streams travel back; what a single call cannot hide is its first
// piece's H2D and its last piece's coder chain (8 x block_size dependent steps per lane whatever the block count) and D2H.
//   - calls that w3_encode_submit would run synchronously (lane-per-block specs, slot leaves on hash maps in HBM): one piece — they
//     take hundreds of milliseconds per GB, PCIe is a few percent of that;
//   - up to W3_FREE_RUN4_BLOCKS blocks: one piece (four coders of such pieces overlap, but one call has only one);
//   - beyond: pieces of at most W3_FREE_RUN4_BLOCKS blocks, equal in size — the four-in-flight regime of DESIGN.md 3.3
//     (measured at 1e9 B from pinned memory, tools/host_api_rate.py: DESIGN.md section 5).
// W3_OPT_HOST_CHUNK_BLOCKS overrides the piece size (tests: ragged pieces; measurements).
// blocks per device call of a host-buffer entry point whose input exceeds what one device call handles (check_args): 2 GiB worth
static size_t host_call_cap_blocks(size_t block_size) { return std::max<size_t>(1, ((size_t)1 << 31) / block_size); }
// ... and of w3_decode_blocks, the ranges calls and AC over Huffman's host-buffer calls, which go through in runs of whole blocks, one device call each
static size_t host_run_blocks(const w3_ctx *ctx, size_t block_size) { return ctx->host_chunk_blocks ? (size_t)ctx->host_chunk_blocks : host_call_cap_blocks(block_size); }

static size_t host_chunk_blocks(const w3_ctx *ctx, const ParsedSpec &ps, size_t nb, size_t block_size, size_t n) {
    const size_t cap = host_call_cap_blocks(block_size);   // (a host buffer of any length goes through in pieces, as the reference streams any length: main.rs:97-109)
    if (!submit_pipelines(ctx, ps, (uint32_t)std::min<size_t>(nb, cap), block_size, std::min(n, cap * block_size))) return std::min(nb, cap);
    if (ctx->host_chunk_blocks) return std::min<size_t>(nb, ctx->host_chunk_blocks);
    if (nb <= W3_FREE_RUN4_BLOCKS) return nb;
    const size_t pieces = (nb + W3_FREE_RUN4_BLOCKS - 1) / W3_FREE_RUN4_BLOCKS;
    return std::min((nb + pieces - 1) / pieces, cap);
}

// one more piece's timing into a call's sums (n_parts counts the pieces; path and n_wide are the last piece's)
static void timing_add(w3_timing &sum, const w3_timing &t) {
    sum.predict_ms += t.predict_ms; sum.coder_ms += t.coder_ms; sum.pack_ms += t.pack_ms; sum.generic_ms += t.generic_ms; sum.total_ms += t.total_ms;
    sum.apm_ms += t.apm_ms; sum.slot_ms += t.slot_ms; sum.achash_ms += t.achash_ms; sum.small_ms += t.small_ms; sum.mix_ms += t.mix_ms; sum.match_ms += t.match_ms;
    for (int w = 0; w < 4; w++) { sum.part_ms[w] += t.part_ms[w]; sum.rank_ms[w] += t.rank_ms[w]; }
    sum.path = t.path; sum.n_wide = t.n_wide; sum.n_parts += 1;
    sum.n_coder_launches += t.n_coder_launches; sum.coder_bytes += t.coder_bytes; sum.predict_bytes += t.predict_bytes;
    sum.n_recoded_blocks += t.n_recoded_blocks; sum.n_slot_launches += t.n_slot_launches; sum.n_lds_faults += t.n_lds_faults;
}

extern "C" int w3_encode_blocks(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, size_t block_size, uint8_t *out,
                                size_t out_cap, size_t *out_len, uint32_t *block_lens) {
    int rc = check_args(ctx, n, block_size, false);   // (any length: the pieces below are the device calls, each under the per-call limit)
    if (rc) return rc;
    if (out_len) *out_len = 0;
    const size_t nb = (n + block_size - 1) / block_size;
    if (nb == 0) return w3_spec_validate(spec);
    if (!in || !block_lens || !out_len) return W3_E_INVALID;
    if ((rc = jobs_idle(ctx))) return rc;
    ParsedSpec ps;
    if ((rc = parse_spec(spec, ps))) { ctx->err = "malformed model spec"; return rc; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t cb = host_chunk_blocks(ctx, ps, nb, block_size, n);
    // one number for the verification's rotation, taken by every piece: with a number per piece, the pieces of equal shape would share
    // one count and each would only ever see every k-th rotation (k pieces per call)
    const int64_t vcall = (int64_t)verify_call(ctx, n, block_size);
    // The pieces in flight, oldest first.  A piece's streams go to `out` at the sum of the earlier pieces' sizes, known when it is
    // waited for; once the caller's buffer is full the later pieces are still encoded (*out_len must hold the size needed) but
    // only their length tables are fetched.
    int q[W3_MAX_HOST_JOBS], qn = 0;
    size_t off = 0;
    int first_err = W3_OK;
    w3_timing sum;
    memset(&sum, 0, sizeof sum);
    auto wait_oldest = [&]() {
        const int hjob = q[0];
        for (int k = 1; k < qn; k++) q[k - 1] = q[k];
        qn--;
        size_t len = 0;
        const bool room = first_err == W3_OK && out && off <= out_cap;
        const int r = host_wait_core(ctx, hjob, room ? out + off : nullptr, room ? out_cap - off : 0, &len);
        off += len;
        if (r != W3_OK && first_err == W3_OK) first_err = r;
        timing_add(sum, ctx->timing);
    };
    // Equal pieces.  (A half-size first and last piece — the call's first H2D + predict phase and its last predict + APM overlap nothing —
    // was measured: 97.6 against 96.9 ms at 1e9 B, 91.8 against 53.4 ms at 4e8 B; profiles/r4_host_path/.)
    for (size_t b0 = 0; b0 < nb; b0 += cb) {
        const size_t lo = b0 * block_size, hi = std::min(n, (b0 + cb) * block_size);
        // (an error that is not "out of room" ends the call: nothing more is submitted, what is in flight is drained below)
        if (first_err != W3_OK && first_err != W3_E_NOSPACE) break;
        while (qn >= host_depth(spec, hi - lo, block_size)) wait_oldest();
        if (first_err != W3_OK && first_err != W3_E_NOSPACE) break;
        int hjob = -1;
        rc = host_submit_core(ctx, spec, ps, in + lo, hi - lo, block_size, nullptr, 0, block_lens + b0, &hjob, vcall);
        if (rc) { if (first_err == W3_OK) first_err = rc; break; }
        q[qn++] = hjob;
    }
    while (qn) wait_oldest();
    ctx->timing = sum;
    if (first_err != W3_OK && first_err != W3_E_NOSPACE) return first_err;
    *out_len = off;
    if (first_err == W3_E_NOSPACE || off > out_cap || !out) { ctx->err = "out_cap too small"; return W3_E_NOSPACE; }
    return W3_OK;
}

// The host-buffer decoders behind their argument checks (nblocks == ceil(orig_len / block_size) >= 1): any length, in runs of whole blocks.  Per run the
// streams and their lengths go to the device, dev(d_in, in_len, d_lens, nblocks, orig_len, d_out) — the family's device entry point — decodes, the bytes come back.
// chk != nullptr (the *_checked calls): after each run's decode the run's part of chk->crc goes up and the decoded bytes are verified on the
// device before they travel; every run is decoded and verified, and the report covers all of them.
template <class Dev>
static int host_decode_runs(w3_ctx *ctx, const uint8_t *in, size_t in_len, const uint32_t *block_lens, size_t nblocks, size_t block_size, uint64_t orig_len,
                            uint8_t *out, Dev &&dev, w3_check *chk = nullptr) {
    const size_t run = host_run_blocks(ctx, block_size);
    uint64_t coff = 0;
    CrcReport rep;
    for (size_t b0 = 0; b0 < nblocks; b0 += run) {
        const size_t b1 = std::min(nblocks, b0 + run);
        uint64_t clen = 0;
        for (size_t b = b0; b < b1; b++) clen += block_lens[b];
        if (coff + clen > in_len) { ctx->err = "block length table claims " + std::to_string(coff + clen) + " compressed bytes, the buffer holds " + std::to_string(in_len); return W3_E_FORMAT; }
        const uint64_t o0 = (uint64_t)b0 * block_size, o1 = std::min<uint64_t>(orig_len, (uint64_t)b1 * block_size);
        ENSURE(ctx, ctx->io_in, std::max<size_t>((size_t)clen, 16));
        ENSURE(ctx, ctx->io_out, (size_t)(o1 - o0));
        ENSURE(ctx, ctx->lens, (b1 - b0) * 4);
        HIPCHK(ctx, hipMemcpy(ctx->io_in.p, in + coff, (size_t)clen, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(ctx->lens.p, block_lens + b0, (b1 - b0) * 4, hipMemcpyHostToDevice));
        if (const int rc = dev((const uint8_t *)ctx->io_in.p, (size_t)clen, (const uint32_t *)ctx->lens.p, b1 - b0, o1 - o0, (uint8_t *)ctx->io_out.p)) return rc;
        if (chk) {
            ENSURE(ctx, ctx->crc_tab, (b1 - b0) * 4);
            HIPCHK(ctx, hipMemcpyAsync(ctx->crc_tab.p, chk->crc + b0, (b1 - b0) * 4, hipMemcpyHostToDevice, ctx->stream));
            if (const int rc = crc_enqueue(ctx, ctx->stream, (const uint8_t *)ctx->io_out.p, o1 - o0, (uint32_t)block_size, nullptr, b1 - b0,
                                           (uint32_t)std::min<uint64_t>(block_size, o1 - o0), nullptr, (const uint32_t *)ctx->crc_tab.p, true)) return rc;
            if (const int rc = crc_fetch(ctx, ctx->stream)) return rc;
        }
        HIPCHK(ctx, hipMemcpy(out + o0, ctx->io_out.p, (size_t)(o1 - o0), hipMemcpyDeviceToHost));   // (waits for the context's blocking stream too)
        if (chk) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); rep.add(b0 + ctx->crc_res[0], ctx->crc_res[1]); }
        coff += clen;
    }
    return chk ? rep.finish(ctx, chk) : W3_OK;
}

// CRC-32 of every block of a host buffer of any length: up in runs of whole blocks (as host_decode_runs), the table back run by run.
extern "C" int w3_crc32_blocks(w3_ctx *ctx, const uint8_t *in, size_t n, size_t block_size, uint32_t *crc) {
    int rc = check_args(ctx, n, block_size, false);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;
    if (n == 0) return W3_OK;
    if (!in || !crc) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = (n + block_size - 1) / block_size, run = host_run_blocks(ctx, block_size);
    for (size_t b0 = 0; b0 < nb; b0 += run) {
        const size_t b1 = std::min(nb, b0 + run);
        const uint64_t o0 = (uint64_t)b0 * block_size, o1 = std::min<uint64_t>(n, (uint64_t)b1 * block_size);
        ENSURE(ctx, ctx->io_in, (size_t)(o1 - o0));
        ENSURE(ctx, ctx->crc_tab, (b1 - b0) * 4);
        HIPCHK(ctx, hipMemcpyAsync(ctx->io_in.p, in + o0, (size_t)(o1 - o0), hipMemcpyHostToDevice, ctx->stream));
        if ((rc = crc_enqueue(ctx, ctx->stream, (const uint8_t *)ctx->io_in.p, o1 - o0, (uint32_t)block_size, nullptr, b1 - b0,
                              (uint32_t)std::min<uint64_t>(block_size, o1 - o0), (uint32_t *)ctx->crc_tab.p, nullptr, false))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(crc + b0, ctx->crc_tab.p, (b1 - b0) * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return W3_OK;
}

// ---------------------------------------------------------------------------
// table preparation on the device (w3_prep.h): the byte histogram and StationaryModel::new
// ---------------------------------------------------------------------------
#define W3_PREP_WS_COUNTS 0u                                      // 256 uint64: the histogram
#define W3_PREP_WS_STATE 2048u                                    // 24 uint32: (c0, c1) of the 8 positions, then their halvings
#define W3_PREP_WS_PARTIAL 4096u                                  // W3_HIST_MAX_WG x 256 uint32: the workgroups' partials
#define W3_PREP_WS_TILES (4096u + W3_HIST_MAX_WG * 1024u)         // 8 uint16 per tile of the stationary walk
#define W3_PREP_NOMINAL_BLOCK 65536u                              // the "block" of these calls' argument checks and of the staged forms' pieces

static int prep_ensure(w3_ctx *ctx, uint64_t n) {
    ENSURE(ctx, ctx->prep_ws, (size_t)(W3_PREP_WS_TILES + ((n + 15u) / W3_STAT_TILE + 1u) * 16u));
    return W3_OK;
}

// the histogram of d_in[0, n) into the workspace's counts (n > 0; does not synchronise).  rep: the copies per counter (W3_HIST_REP
// everywhere but in the measurement of w3_table_prep_profile)
static int hist_enqueue(w3_ctx *ctx, hipStream_t s, const uint8_t *d_in, uint64_t n, uint32_t rep = W3_HIST_REP, hipEvent_t ev_mid = nullptr) {
    uint8_t *ws = (uint8_t *)ctx->prep_ws.p;
    uint32_t *partial = (uint32_t *)(ws + W3_PREP_WS_PARTIAL);
    const uint32_t wg = hist_workgroups(n);
    switch (rep) {
    case 1: hipLaunchKernelGGL((k_hist256<1u>), dim3(wg), dim3(256), 0, s, d_in, n, partial); break;
    case 2: hipLaunchKernelGGL((k_hist256<2u>), dim3(wg), dim3(256), 0, s, d_in, n, partial); break;
    case 4: hipLaunchKernelGGL((k_hist256<4u>), dim3(wg), dim3(256), 0, s, d_in, n, partial); break;
    case 8: hipLaunchKernelGGL((k_hist256<8u>), dim3(wg), dim3(256), 0, s, d_in, n, partial); break;
    case 16: hipLaunchKernelGGL((k_hist256<16u>), dim3(wg), dim3(256), 0, s, d_in, n, partial); break;
    default: ctx->err = "copies per counter: 1, 2, 4, 8 or 16"; return W3_E_INVALID;
    }
    HIPCHK(ctx, hipGetLastError());
    if (ev_mid) HIPCHK(ctx, hipEventRecord(ev_mid, s));
    hipLaunchKernelGGL(k_hist256_sum, dim3(256), dim3(64), 0, s, (const uint32_t *)partial, wg, (uint64_t *)(ws + W3_PREP_WS_COUNTS));
    HIPCHK(ctx, hipGetLastError());
    return W3_OK;
}

// the stationary walk over d_in[0, n) from the state in the workspace to the state in the workspace (n > 0; does not synchronise)
static int stat_enqueue(w3_ctx *ctx, hipStream_t s, const uint8_t *d_in, uint64_t n, hipEvent_t ev_mid = nullptr) {
    uint8_t *ws = (uint8_t *)ctx->prep_ws.p;
    uint16_t *ones8 = (uint16_t *)(ws + W3_PREP_WS_TILES);
    const uint64_t ntiles = stat_tiles(prep_window(d_in, n));
    hipLaunchKernelGGL(k_stat_count, dim3((uint32_t)std::min<uint64_t>((ntiles + 3) / 4, 4096)), dim3(256), 0, s, d_in, n, ones8);
    HIPCHK(ctx, hipGetLastError());
    if (ev_mid) HIPCHK(ctx, hipEventRecord(ev_mid, s));
    hipLaunchKernelGGL(k_stat_walk, dim3(8), dim3(64), 0, s, d_in, n, (const uint16_t *)ones8, (uint32_t *)(ws + W3_PREP_WS_STATE));
    HIPCHK(ctx, hipGetLastError());
    return W3_OK;
}
static void stat_table_of(const uint32_t state[24], uint16_t table[8]) {
    for (int i = 0; i < 8; i++) table[i] = stat_table_entry(state[2 * i], state[2 * i + 1]);
}

// the checks the calls share (block_size: the nominal block, so that check_args' limits are the family's)
static int prep_args(w3_ctx *ctx, const void *in, size_t n, const void *out, bool one_device) {
    int rc = check_args(ctx, n, W3_PREP_NOMINAL_BLOCK, one_device);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;   // (the workspace is the context's)
    if (!out || (!in && n)) return W3_E_INVALID;
    return W3_OK;
}

extern "C" int w3_histogram_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t counts[256], void *stream) {
    int rc = prep_args(ctx, d_in, n, counts, true);
    if (rc) return rc;
    memset(counts, 0, 256 * sizeof(uint64_t));
    if (n == 0) return W3_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = prep_ensure(ctx, 0))) return rc;
    if ((rc = hist_enqueue(ctx, s, d_in, n))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(counts, (uint8_t *)ctx->prep_ws.p + W3_PREP_WS_COUNTS, 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return W3_OK;
}

// A host buffer of any length: up through ctx->io_in in pieces of host_run_blocks nominal 64 KiB blocks (W3_OPT_HOST_CHUNK_BLOCKS: ragged
// pieces for the tests), the pieces' counts added up in 64 bits.
extern "C" int w3_histogram(w3_ctx *ctx, const uint8_t *in, size_t n, uint64_t counts[256]) {
    int rc = prep_args(ctx, in, n, counts, false);
    if (rc) return rc;
    memset(counts, 0, 256 * sizeof(uint64_t));
    if (n == 0) return W3_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t piece = host_run_blocks(ctx, W3_PREP_NOMINAL_BLOCK) * (size_t)W3_PREP_NOMINAL_BLOCK;
    if ((rc = prep_ensure(ctx, 0))) return rc;
    ENSURE(ctx, ctx->io_in, std::min(n, piece));
    uint64_t part[256];
    for (size_t o0 = 0; o0 < n; o0 += piece) {
        const size_t len = std::min(piece, n - o0);
        HIPCHK(ctx, hipMemcpyAsync(ctx->io_in.p, in + o0, len, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = hist_enqueue(ctx, ctx->stream, (const uint8_t *)ctx->io_in.p, len))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(part, (uint8_t *)ctx->prep_ws.p + W3_PREP_WS_COUNTS, sizeof part, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (int v = 0; v < 256; v++) counts[v] += part[v];
    }
    return W3_OK;
}

extern "C" int w3_stationary_table_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, uint16_t table[8], void *stream) {
    int rc = prep_args(ctx, d_in, n, table, true);
    if (rc) return rc;
    uint32_t state[24] = {0};
    if (n) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        if ((rc = prep_ensure(ctx, n))) return rc;
        uint8_t *d_state = (uint8_t *)ctx->prep_ws.p + W3_PREP_WS_STATE;
        HIPCHK(ctx, hipMemsetAsync(d_state, 0, sizeof state, s));
        if ((rc = stat_enqueue(ctx, s, d_in, n))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(state, d_state, sizeof state, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    stat_table_of(state, table);
    return W3_OK;
}

// The same from a host buffer of any length, staged as w3_histogram stages: the walk's state stays on the device from piece to piece.
extern "C" int w3_stationary_table_staged(w3_ctx *ctx, const uint8_t *in, size_t n, uint16_t table[8]) {
    int rc = prep_args(ctx, in, n, table, false);
    if (rc) return rc;
    uint32_t state[24] = {0};
    if (n) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        const size_t piece = host_run_blocks(ctx, W3_PREP_NOMINAL_BLOCK) * (size_t)W3_PREP_NOMINAL_BLOCK;
        if ((rc = prep_ensure(ctx, std::min(n, piece)))) return rc;
        ENSURE(ctx, ctx->io_in, std::min(n, piece));
        uint8_t *d_state = (uint8_t *)ctx->prep_ws.p + W3_PREP_WS_STATE;
        HIPCHK(ctx, hipMemsetAsync(d_state, 0, sizeof state, ctx->stream));
        for (size_t o0 = 0; o0 < n; o0 += piece) {
            const size_t len = std::min(piece, n - o0);
            HIPCHK(ctx, hipMemcpyAsync(ctx->io_in.p, in + o0, len, hipMemcpyHostToDevice, ctx->stream));
            if ((rc = stat_enqueue(ctx, ctx->stream, (const uint8_t *)ctx->io_in.p, len))) return rc;
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the next piece overwrites io_in)
        }
        HIPCHK(ctx, hipMemcpy(state, d_state, sizeof state, hipMemcpyDeviceToHost));
    }
    stat_table_of(state, table);
    return W3_OK;
}

// Both preparations of d_in[0, n) once, every kernel between HIP events (tools/table_prep_rate.py).
extern "C" int w3_table_prep_profile(w3_ctx *ctx, const uint8_t *d_in, size_t n, uint32_t hist_rep, w3_prep_profile *out) {
    int rc = prep_args(ctx, d_in, n, out, true);
    if (rc) return rc;
    memset(out, 0, sizeof *out);
    uint32_t state[24] = {0};
    if (n) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        if ((rc = prep_ensure(ctx, n))) return rc;
        uint8_t *ws = (uint8_t *)ctx->prep_ws.p;
        hipEvent_t ev[5] = {};
        for (auto &e : ev) HIPCHK(ctx, hipEventCreate(&e));
        HIPCHK(ctx, hipMemsetAsync(ws + W3_PREP_WS_STATE, 0, sizeof state, s));
        HIPCHK(ctx, hipEventRecord(ev[0], s));
        rc = hist_enqueue(ctx, s, d_in, n, hist_rep, ev[1]);
        if (!rc) HIPCHK(ctx, hipEventRecord(ev[2], s));
        if (!rc) rc = stat_enqueue(ctx, s, d_in, n, ev[3]);
        if (!rc) HIPCHK(ctx, hipEventRecord(ev[4], s));
        if (!rc) {
            HIPCHK(ctx, hipMemcpyAsync(out->counts, ws + W3_PREP_WS_COUNTS, sizeof out->counts, hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipMemcpyAsync(state, ws + W3_PREP_WS_STATE, sizeof state, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (!rc) {
            float *ms[4] = {&out->hist_ms, &out->hist_sum_ms, &out->stat_count_ms, &out->stat_walk_ms};
            for (int k = 0; k < 4; k++) HIPCHK(ctx, hipEventElapsedTime(ms[k], ev[k], ev[k + 1]));
        }
        for (auto &e : ev) (void)hipEventDestroy(e);
        if (rc) return rc;
    }
    stat_table_of(state, out->table);
    for (int i = 0; i < 8; i++) out->halvings[i] = state[16 + i];
    return W3_OK;
}

static int decode_blocks_host(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, const uint32_t *block_lens, size_t nblocks,
                             size_t block_size, uint64_t orig_len, uint8_t *out, w3_check *chk) {
    int rc = check_args(ctx, (size_t)orig_len, block_size, false);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;
    if (nblocks == 0 && orig_len == 0) return w3_spec_validate(spec);
    if (!in || !block_lens || !out) return W3_E_INVALID;
    if ((uint64_t)nblocks != (orig_len + block_size - 1) / block_size) { ctx->err = "nblocks does not match orig_len/block_size"; return W3_E_INVALID; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return host_decode_runs(ctx, in, in_len, block_lens, nblocks, block_size, orig_len, out, [&](const uint8_t *d_in, size_t len, const uint32_t *d_lens, size_t nb, uint64_t olen, uint8_t *d_out) {
        return w3_decode_blocks_device(ctx, spec, d_in, len, d_lens, nb, block_size, olen, d_out, ctx->stream);
    }, chk);
}
extern "C" int w3_decode_blocks(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, const uint32_t *block_lens, size_t nblocks,
                                size_t block_size, uint64_t orig_len, uint8_t *out) {
    return decode_blocks_host(ctx, spec, in, in_len, block_lens, nblocks, block_size, orig_len, out, nullptr);
}
extern "C" int w3_decode_blocks_checked(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                                        size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *out, w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    if (const int rc = check_arg(ctx, chk)) return rc;
    return decode_blocks_host(ctx, spec, in, in_len, block_lens, nblocks, block_size, orig_len, out, chk);
}

// ---------------------------------------------------------------------------
// random access: byte ranges of the block container (w3_ranges.h plans them)
// ---------------------------------------------------------------------------
static_assert(sizeof(RangeJob) == sizeof(DecodeJob) && offsetof(RangeJob, dst) == offsetof(DecodeJob, dst), "w3_ranges.h jobs are the decoders' DecodeJob");
static_assert(sizeof(w3_range) == 16, "ABI struct layout");

static int ranges_invalid(w3_ctx *ctx, uint64_t orig_len, size_t block_size, size_t nblocks) {
    ctx->err = (uint64_t)nblocks != (orig_len + block_size - 1) / block_size ? "nblocks does not match orig_len/block_size"
                                                                            : "a range runs past orig_len";
    return W3_E_INVALID;
}

// The job table and the gather's pieces of a plan, one after the other: jobs at 0, pieces at *chunks_off (16-byte aligned).
static std::vector<uint8_t> ranges_meta(const std::vector<RangeJob> &jobs, const std::vector<RangePiece> &chunks, size_t &chunks_off) {
    const size_t jb = jobs.size() * sizeof(RangeJob);
    chunks_off = (jb + 15) / 16 * 16;
    std::vector<uint8_t> m(chunks_off + chunks.size() * sizeof(RangePiece));
    if (jb) memcpy(m.data(), jobs.data(), jb);
    if (!chunks.empty()) memcpy(m.data() + chunks_off, chunks.data(), chunks.size() * sizeof(RangePiece));
    return m;
}

// The decoder behind a ranges call: a model spec (w3_decode_ranges*), or AC over Huffman's table and ctx_bits (w3_aoh_decode_ranges*).
struct RangeDec {
    const ParsedSpec *ps = nullptr;
    const w3_huff_code *aoh_code = nullptr; uint8_t aoh_ctx_bits = 0;
    // the *_checked calls: every touched block is decoded whole (widen_to_whole_blocks) and verified in the staging buffer before the gather
    w3_check *chk = nullptr;
    CrcReport *rep = nullptr;
};
// the verify's segment list of a widened plan, appended to a call's metadata (16-byte aligned; *segs_off = where)
static void ranges_crc_segs(std::vector<uint8_t> &meta, const RangePlan &p, const uint32_t *crc, size_t &segs_off) {
    segs_off = (meta.size() + 15) / 16 * 16;
    meta.resize(segs_off + p.blocks.size() * sizeof(CrcSeg));
    CrcSeg *sg = (CrcSeg *)(meta.data() + segs_off);
    for (size_t k = 0; k < p.blocks.size(); k++) sg[k] = CrcSeg{p.bdst[k], p.blen[k], crc[p.blocks[k]]};
}
// (the AOH decoders live with their family, below)
static int aoh_decode_run(w3_ctx *ctx, hipStream_t s, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_cin, const uint32_t *d_lens, uint32_t nb,
                          size_t block_size, uint64_t orig_len, uint8_t *d_out, const DecodeJob *d_jobs, uint32_t n_jobs, uint32_t max_job_len, bool spec);
static bool aoh_ranges_take_spec(const w3_ctx *ctx, uint8_t ctx_bits);

// Decode the jobs (d_jobs[n_jobs], stream indices into d_lens[nb] / d_cin; the longest decodes max_job_len bytes) into the staging
// buffer, then gather the pieces (d_chunks[n_chunks], at most W3_GATHER_PIECE_MAX bytes each) into d_out.  d_segs != nullptr (a checked
// call): between the two, the n_jobs segments of the staging buffer are verified and the result is on its way to ctx->crc_res.
static int ranges_run(w3_ctx *ctx, hipStream_t s, const RangeDec &rd, const uint8_t *d_cin, const uint32_t *d_lens, uint32_t nb, size_t block_size,
                      uint64_t orig_len, const DecodeJob *d_jobs, uint32_t n_jobs, uint32_t max_job_len, const RangePiece *d_chunks, uint32_t n_chunks,
                      uint64_t staging, uint8_t *d_out, const CrcSeg *d_segs = nullptr) {
    ENSURE(ctx, ctx->rg_stage, (size_t)staging + 16);   // (k_gather_pieces reads up to 3 bytes past a piece)
    uint8_t *d_stage = (uint8_t *)ctx->rg_stage.p;
    LaneIo io;
    io.cin = d_cin; io.clens = d_lens; io.dout = d_stage; io.jobs = d_jobs; io.n_jobs = n_jobs;
    const int rc = !rd.ps ? aoh_decode_run(ctx, s, rd.aoh_code, rd.aoh_ctx_bits, d_cin, d_lens, nb, block_size, orig_len, d_stage, d_jobs, n_jobs, max_job_len,
                                           aoh_ranges_take_spec(ctx, rd.aoh_ctx_bits))
                          : lane_run<true>(ctx, s, *rd.ps, block_size, orig_len, nb, io);
    if (rc) return rc;
    if (d_segs) {
        if (const int r = crc_enqueue(ctx, s, d_stage, staging, (uint32_t)block_size, d_segs, n_jobs, max_job_len, nullptr, nullptr, true)) return r;
        if (const int r = crc_fetch(ctx, s)) return r;
    }
    hipLaunchKernelGGL(k_gather_pieces, dim3(std::min<uint32_t>(n_chunks, 4096u)), dim3(256), 0, s, (const uint8_t *)d_stage, d_chunks, n_chunks, d_out);
    HIPCHK(ctx, hipGetLastError());
    return W3_OK;
}

// w3_decode_ranges_device / w3_aoh_decode_ranges_device behind their argument checks (*out_len is 0 on entry)
static int ranges_device(w3_ctx *ctx, const RangeDec &rd, const uint8_t *d_in, size_t in_len, const uint32_t *d_block_lens, size_t nblocks, size_t block_size,
                         uint64_t orig_len, const w3_range *ranges, size_t n_ranges, uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream) {
    int rc;
    RangePlan p;
    if (plan_ranges(orig_len, block_size, nblocks, ranges, n_ranges, p)) return ranges_invalid(ctx, orig_len, block_size, nblocks);
    *out_len = (size_t)p.out_len;
    if (p.out_len > out_cap) { ctx->err = "out_cap too small"; return W3_E_NOSPACE; }
    if (p.out_len == 0) return W3_OK;
    if (!d_in || !d_block_lens || !d_out) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (rd.ps && (rc = stage_huff(ctx, s, *rd.ps))) return rc;
    if ((rc = check_len_table(ctx, s, d_block_lens, (uint32_t)nblocks, in_len))) return rc;
    if (rd.chk) widen_to_whole_blocks(p, orig_len, block_size);
    const std::vector<RangePiece> chunks = gather_chunks(p, W3_GATHER_PIECE_MAX);
    size_t coff = 0, segs_off = 0;
    std::vector<uint8_t> meta = ranges_meta(p.jobs, chunks, coff);
    if (rd.chk) ranges_crc_segs(meta, p, rd.chk->crc, segs_off);
    ENSURE(ctx, ctx->rg_meta, meta.size());
    HIPCHK(ctx, hipMemcpyAsync(ctx->rg_meta.p, meta.data(), meta.size(), hipMemcpyHostToDevice, s));
    rc = ranges_run(ctx, s, rd, d_in, d_block_lens, (uint32_t)nblocks, block_size, orig_len, (const DecodeJob *)ctx->rg_meta.p, (uint32_t)p.jobs.size(),
                    p.jobs[0].len, (const RangePiece *)((uint8_t *)ctx->rg_meta.p + coff), (uint32_t)chunks.size(), p.staging, d_out,
                    rd.chk ? (const CrcSeg *)((uint8_t *)ctx->rg_meta.p + segs_off) : nullptr);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));   // (meta: pageable memory of this frame)
    if (rd.chk && ctx->crc_res[1]) rd.rep->add(p.blocks[(size_t)ctx->crc_res[0]], ctx->crc_res[1]);
    return W3_OK;
}

static int decode_ranges_device_any(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t in_len, const uint32_t *d_block_lens,
                                    size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges,
                                    uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream, w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    if (out_len) *out_len = 0;
    int rc = check_args(ctx, (size_t)orig_len, block_size);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;   // (job 0's HuffHistory tables, length scan and model tables)
    ParsedSpec ps;
    if ((rc = parse_spec(spec, ps))) { ctx->err = "malformed model spec"; return rc; }
    if (!out_len) return W3_E_INVALID;
    RangeDec rd;
    CrcReport rep;
    rd.ps = &ps; rd.chk = chk; rd.rep = &rep;
    rc = ranges_device(ctx, rd, d_in, in_len, d_block_lens, nblocks, block_size, orig_len, ranges, n_ranges, d_out, out_cap, out_len, stream);
    return rc || !chk ? rc : rep.finish(ctx, chk);
}
extern "C" int w3_decode_ranges_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t in_len, const uint32_t *d_block_lens,
                                       size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges,
                                       uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream) {
    return decode_ranges_device_any(ctx, spec, d_in, in_len, d_block_lens, nblocks, block_size, orig_len, ranges, n_ranges, d_out, out_cap, out_len, stream, nullptr);
}
extern "C" int w3_decode_ranges_device_checked(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t in_len, const uint32_t *d_block_lens,
                                               size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges,
                                               uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream, w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    if (out_len) *out_len = 0;
    if (const int rc = check_arg(ctx, chk)) return rc;
    return decode_ranges_device_any(ctx, spec, d_in, in_len, d_block_lens, nblocks, block_size, orig_len, ranges, n_ranges, d_out, out_cap, out_len, stream, chk);
}

// One device call of the host variant: only the selected blocks' streams go over PCIe, with the compact length table, the jobs (naming
// streams by their index in that table) and the gather's pieces — all in one pinned buffer, one H2D copy — then one D2H copy of the
// packed output.  The ranges were validated by the caller; the length table's total was checked against in_len.
static int ranges_host_one(w3_ctx *ctx, const RangeDec &rd, const uint8_t *in, const uint32_t *block_lens, size_t nblocks, size_t block_size,
                           uint64_t orig_len, const w3_range *ranges, size_t n_ranges, uint8_t *out) {
    RangePlan p;
    if (plan_ranges(orig_len, block_size, nblocks, ranges, n_ranges, p)) return ranges_invalid(ctx, orig_len, block_size, nblocks);
    if (p.out_len == 0) return W3_OK;
    const size_t nd = p.blocks.size();
    std::vector<uint64_t> soff(nd);   // the selected streams' offsets in `in`
    {
        uint64_t c = 0;
        size_t k = 0;
        for (size_t b = 0; b < nblocks && k < nd; b++) {
            if (b == p.blocks[k]) soff[k++] = c;
            c += block_lens[b];
        }
    }
    uint64_t sbytes = 0;
    for (size_t k = 0; k < nd; k++) sbytes += block_lens[p.blocks[k]];
    if (rd.chk) widen_to_whole_blocks(p, orig_len, block_size);
    const std::vector<RangePiece> chunks = gather_chunks(p, W3_GATHER_PIECE_MAX);
    size_t coff = 0, segs_off = 0;
    std::vector<uint8_t> meta = ranges_meta(compact_jobs(p), chunks, coff);
    if (rd.chk) ranges_crc_segs(meta, p, rd.chk->crc, segs_off);
    const size_t lens_off = (meta.size() + 15) / 16 * 16, str_off = (lens_off + nd * 4 + 15) / 16 * 16;
    const size_t bytes = str_off + (size_t)sbytes;
    if (bytes > ctx->h_rg_cap) {
        if (ctx->h_rg) { HIPCHK(ctx, hipHostFree(ctx->h_rg)); ctx->h_rg = nullptr; ctx->h_rg_cap = 0; }
        const size_t want = std::max<size_t>(bytes, 1 << 20);
        if (hipHostMalloc(&ctx->h_rg, want) != hipSuccess) { (void)hipGetLastError(); ctx->h_rg = nullptr; ctx->err = "hipHostMalloc(" + std::to_string(want) + ") failed"; return W3_E_NOMEM; }
        ctx->h_rg_cap = want;
    }
    uint8_t *h = (uint8_t *)ctx->h_rg;
    memcpy(h, meta.data(), meta.size());
    uint32_t *hl = (uint32_t *)(h + lens_off);
    uint64_t o = 0;
    for (size_t k = 0; k < nd; k++) {
        hl[k] = block_lens[p.blocks[k]];
        memcpy(h + str_off + o, in + soff[k], hl[k]);
        o += hl[k];
    }
    hipStream_t s = ctx->stream;
    ENSURE(ctx, ctx->rg_meta, bytes);
    ENSURE(ctx, ctx->io_out, (size_t)p.out_len);
    uint8_t *d = (uint8_t *)ctx->rg_meta.p;
    HIPCHK(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
    int rc = rd.ps ? stage_huff(ctx, s, *rd.ps) : W3_OK;
    if (rc) return rc;
    if ((rc = scan_lens(ctx, s, (const uint32_t *)(d + lens_off), (uint32_t)nd))) return rc;   // (the compact table's total was checked on the host)
    rc = ranges_run(ctx, s, rd, d + str_off, (const uint32_t *)(d + lens_off), (uint32_t)nd, block_size, orig_len, (const DecodeJob *)d, (uint32_t)nd,
                    p.jobs[0].len, (const RangePiece *)(d + coff), (uint32_t)chunks.size(), p.staging, (uint8_t *)ctx->io_out.p,
                    rd.chk ? (const CrcSeg *)(d + segs_off) : nullptr);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->io_out.p, (size_t)p.out_len, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (rd.chk && ctx->crc_res[1]) rd.rep->add(p.blocks[(size_t)ctx->crc_res[0]], ctx->crc_res[1]);
    return W3_OK;
}

// w3_decode_ranges / w3_aoh_decode_ranges behind their argument checks (*out_len is 0 on entry)
static int ranges_host(w3_ctx *ctx, const RangeDec &rd, const uint8_t *in, size_t in_len, const uint32_t *block_lens, size_t nblocks, size_t block_size,
                       uint64_t orig_len, const w3_range *ranges, size_t n_ranges, uint8_t *out, size_t out_cap, size_t *out_len) {
    int rc;
    RangePlan p;
    if (plan_ranges(orig_len, block_size, nblocks, ranges, n_ranges, p)) return ranges_invalid(ctx, orig_len, block_size, nblocks);
    *out_len = (size_t)p.out_len;
    if (p.out_len > out_cap) { ctx->err = "out_cap too small"; return W3_E_NOSPACE; }
    if (p.out_len == 0) return W3_OK;
    if (!in || !block_lens || !out) return W3_E_INVALID;
    uint64_t total = 0;
    for (size_t b = 0; b < nblocks; b++) total += block_lens[b];
    if (total > in_len) { ctx->err = "block length table claims " + std::to_string(total) + " compressed bytes, the buffer holds " + std::to_string(in_len); return W3_E_FORMAT; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // blocks per device call: 2 GiB worth (W3_OPT_HOST_CHUNK_BLOCKS: fewer, for tests), and at most as many bytes of packed output
    const uint64_t capb = host_run_blocks(ctx, block_size);
    if (p.blocks.size() <= capb && p.out_len <= capb * block_size)
        return ranges_host_one(ctx, rd, in, block_lens, nblocks, block_size, orig_len, ranges, n_ranges, out);
    // A larger selection: the ranges are cut into parts of at most capb / 2 blocks' worth (each touches at most capb / 2 + 1 blocks), and
    // runs of consecutive parts go through one device call each while their blocks, counted part by part, and bytes stay within the cap.
    // Consecutive parts are consecutive stretches of the output, so each call writes its packed output straight to its place in `out`.
    const uint64_t part = std::max<uint64_t>(1, capb / 2) * block_size;
    std::vector<w3_range> batch;
    uint64_t bblocks = 0, bbytes = 0, dst = 0;
    auto flush = [&]() -> int {
        if (batch.empty()) return W3_OK;
        const int r = ranges_host_one(ctx, rd, in, block_lens, nblocks, block_size, orig_len, batch.data(), batch.size(), out + dst);
        dst += bbytes;
        batch.clear(); bblocks = 0; bbytes = 0;
        return r;
    };
    for (size_t q = 0; q < n_ranges; q++) {
        const uint64_t end = ranges[q].offset + ranges[q].len;
        for (uint64_t o = ranges[q].offset; o < end; o += part) {
            const w3_range r{o, std::min(part, end - o)};
            const uint64_t rb = (r.offset + r.len - 1) / block_size - r.offset / block_size + 1;
            if (bblocks + rb > capb || bbytes + r.len > capb * block_size)
                if ((rc = flush())) return rc;
            batch.push_back(r); bblocks += rb; bbytes += r.len;
        }
    }
    return flush();
}

static int decode_ranges_any(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                             size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges,
                             uint8_t *out, size_t out_cap, size_t *out_len, w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    if (out_len) *out_len = 0;
    int rc = check_args(ctx, (size_t)orig_len, block_size, false);   // (any length: a large selection goes through in several device calls)
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;
    ParsedSpec ps;
    if ((rc = parse_spec(spec, ps))) { ctx->err = "malformed model spec"; return rc; }
    if (!out_len) return W3_E_INVALID;
    RangeDec rd;
    CrcReport rep;
    rd.ps = &ps; rd.chk = chk; rd.rep = &rep;
    rc = ranges_host(ctx, rd, in, in_len, block_lens, nblocks, block_size, orig_len, ranges, n_ranges, out, out_cap, out_len);
    return rc || !chk ? rc : rep.finish(ctx, chk);
}
extern "C" int w3_decode_ranges(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                                size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges,
                                uint8_t *out, size_t out_cap, size_t *out_len) {
    return decode_ranges_any(ctx, spec, in, in_len, block_lens, nblocks, block_size, orig_len, ranges, n_ranges, out, out_cap, out_len, nullptr);
}
extern "C" int w3_decode_ranges_checked(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                                        size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges,
                                        uint8_t *out, size_t out_cap, size_t *out_len, w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    if (out_len) *out_len = 0;
    if (const int rc = check_arg(ctx, chk)) return rc;
    return decode_ranges_any(ctx, spec, in, in_len, block_lens, nblocks, block_size, orig_len, ranges, n_ranges, out, out_cap, out_len, chk);
}

// ---------------------------------------------------------------------------
// one process, several GPUs: contiguous block ranges, one host thread and context per device
// ---------------------------------------------------------------------------
extern "C" int w3_shard_range(size_t nblocks, int world, int rank, size_t *first_block, size_t *end_block) {
    if (world <= 0 || rank < 0 || rank >= world || !first_block || !end_block) return W3_E_INVALID;
    *first_block = (size_t)((unsigned __int128)nblocks * (unsigned)rank / (unsigned)world);
    *end_block = (size_t)((unsigned __int128)nblocks * (unsigned)(rank + 1) / (unsigned)world);
    return W3_OK;
}

extern "C" int w3_encode_blocks_sharded(w3_ctx *const *ctxs, int n_ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, size_t block_size,
                                        uint8_t *out, size_t out_cap, size_t *out_len, uint32_t *block_lens) {
    if (!ctxs || n_ctx <= 0 || !out_len) return W3_E_INVALID;
    for (int r = 0; r < n_ctx; r++) {
        if (!ctxs[r]) return W3_E_INVALID;
        for (int q = 0; q < r; q++)
            if (ctxs[q] == ctxs[r]) { ctxs[0]->err = "the same context appears twice in ctxs[] (a context is not thread-safe)"; return W3_E_INVALID; }
    }
    *out_len = 0;
    int rc = check_args(ctxs[0], n, block_size, false);   // (the size limit of one call applies to each shard)
    if (rc) return rc;
    const size_t nb = (n + block_size - 1) / block_size;
    if (nb == 0) return w3_spec_validate(spec);
    if (!in || !block_lens) return W3_E_INVALID;
    struct Shard { size_t lo = 0, hi = 0, b0 = 0; std::vector<uint8_t> buf; size_t len = 0; int rc = W3_OK; };
    std::vector<Shard> sh(n_ctx);
    std::vector<std::thread> th;
    for (int r = 0; r < n_ctx; r++) {
        size_t b0, b1;
        (void)w3_shard_range(nb, n_ctx, r, &b0, &b1);
        sh[r].b0 = b0; sh[r].lo = std::min(b0 * block_size, n); sh[r].hi = std::min(b1 * block_size, n);
        if (sh[r].hi == sh[r].lo) continue;
        th.emplace_back([&, r]() {
            Shard &x = sh[r];
            const size_t m = x.hi - x.lo;
            size_t cap = 2 * m + 64 * ((m + block_size - 1) / block_size) + 64;   // realistic bound; grown to the reported need on W3_E_NOSPACE
            for (int attempt = 0; attempt < 2; attempt++) {
                x.buf.resize(cap);
                x.rc = w3_encode_blocks(ctxs[r], spec, in + x.lo, m, block_size, x.buf.data(), cap, &x.len, block_lens + x.b0);
                if (x.rc != W3_E_NOSPACE || x.len <= cap) break;
                cap = x.len;
            }
        });
    }
    for (auto &t : th) t.join();
    size_t total = 0;
    for (int r = 0; r < n_ctx; r++) {
        if (sh[r].rc) { ctxs[0]->err = "shard " + std::to_string(r) + ": " + (ctxs[r]->err.empty() ? w3_strerror(sh[r].rc) : ctxs[r]->err); return sh[r].rc; }
        total += sh[r].len;
    }
    *out_len = total;
    if (total > out_cap || !out) return W3_E_NOSPACE;
    size_t o = 0;
    for (int r = 0; r < n_ctx; r++) { if (sh[r].len) memcpy(out + o, sh[r].buf.data(), sh[r].len); o += sh[r].len; }
    return W3_OK;
}

// ---------------------------------------------------------------------------
// The same sharding with the data resident on the devices and the gather over xGMI (north star: "RCCL gather over xGMI to
// concatenate per-GPU compressed streams"; SURVEY section 8(e): ncclCommInitAll, sizes all-gather, grouped ncclSend / ncclRecv at
// the offsets of the exclusive scan — RCCL has no gatherv).  One process, one context and one host thread per device.
// ---------------------------------------------------------------------------
struct ShardComms {          // one communicator set per device list, created on first use and kept (ncclCommInitAll is slow)
    std::vector<int> devs;
    std::vector<w3rccl::comm_t> comms;
};
static std::mutex g_comm_mu;
static std::vector<ShardComms *> g_comms;

static ShardComms *shard_comms(const std::vector<int> &devs, std::string &err) {
    std::lock_guard<std::mutex> lk(g_comm_mu);
    for (ShardComms *c : g_comms)
        if (c->devs == devs) return c;
    w3rccl::Api *r = w3rccl::api();
    if (!r->error.empty()) { err = r->error; return nullptr; }
    ShardComms *c = new ShardComms();
    c->devs = devs; c->comms.assign(devs.size(), nullptr);
    const int rc = r->CommInitAll(c->comms.data(), (int)devs.size(), devs.data());
    if (rc != w3rccl::kSuccess) { err = std::string("ncclCommInitAll: ") + r->GetErrorString(rc); delete c; return nullptr; }
    g_comms.push_back(c);
    return c;
}

// The exchange step of a sharded encode: the ranks' totals (RCCL: an all-gather, checked against what the host knows), then the packed
// streams and length tables to the root at the exclusive scan of the totals / block counts.  src_*[r]: rank r's packed streams, length
// table and 8-byte total on ITS device; cm == nullptr: device copies (same device: D2D, other devices: peer copies) instead of RCCL.
// The transfers run on the contexts' own streams (idle while submitted calls are in flight) and have landed when this returns.
static int shard_gather(w3_ctx *const *ctxs, int n_ctx, int root, ShardComms *cm, void *const *src_out, void *const *src_lens, void *const *src_total,
                        const std::vector<size_t> &nbs, const uint64_t *totals, uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens) {
    const bool use_rccl = cm != nullptr;
    w3_ctx *rt = ctxs[root];
    HIPCHK(rt, hipSetDevice(rt->device));
    // 2. the sizes: with RCCL an all-gather of every rank's total (the exchange step's first half, exercised even with one rank).
    // Nothing between ncclGroupStart and ncclGroupEnd may leave this function: an open group would swallow every later RCCL call of
    // this thread.  So whatever can fail for other reasons (allocations, memsets) is done first, and inside a group only RCCL's own
    // return codes are collected.
    if (use_rccl) {
        w3rccl::Api *rc_api = w3rccl::api();
        for (int r = 0; r < n_ctx; r++) {
            w3_ctx *c = ctxs[r];
            HIPCHK(c, hipSetDevice(c->device));
            if (!nbs[r]) HIPCHK(c, hipMemsetAsync(src_total[r], 0, 8, c->stream));   // (holds this rank's total already when the shard was not empty)
            ENSURE(c, c->misc, 8 * (size_t)n_ctx);
        }
        int gs = rc_api->GroupStart();
        const bool opened = gs == w3rccl::kSuccess;
        for (int r = 0; r < n_ctx && gs == w3rccl::kSuccess; r++) {
            (void)hipSetDevice(ctxs[r]->device);   // (a communicator knows its device; set for RCCL versions that look at the current one)
            gs = rc_api->AllGather(src_total[r], ctxs[r]->misc.p, 1, w3rccl::kUint64, cm->comms[r], ctxs[r]->stream);
        }
        const int ge = opened ? rc_api->GroupEnd() : w3rccl::kSuccess;
        if (gs != w3rccl::kSuccess || ge != w3rccl::kSuccess) { ctxs[0]->err = std::string("ncclAllGather: ") + rc_api->GetErrorString(gs != w3rccl::kSuccess ? gs : ge); return W3_E_HIP; }
        std::vector<uint64_t> seen(n_ctx);
        HIPCHK(rt, hipSetDevice(rt->device));
        HIPCHK(rt, hipStreamSynchronize(rt->stream));
        HIPCHK(rt, hipMemcpy(seen.data(), rt->misc.p, 8 * (size_t)n_ctx, hipMemcpyDeviceToHost));
        for (int r = 0; r < n_ctx; r++)
            if (seen[r] != totals[r]) { ctxs[0]->err = "sizes all-gather disagrees with the shards' totals (internal error)"; return W3_E_HIP; }
    }
    uint64_t sum = 0;
    for (int r = 0; r < n_ctx; r++) sum += totals[r];
    if (sum > out_cap) { ctxs[0]->err = "out_cap too small for the gathered streams"; return W3_E_NOSPACE; }

    // 3. the streams and length tables to the root, at the exclusive scan of the totals / block counts
    if (use_rccl) {
        w3rccl::Api *rc_api = w3rccl::api();
        HIPCHK(rt, hipSetDevice(rt->device));
        {   // the root's own shard: a device copy, outside the group
            uint64_t so = 0; size_t lo = 0;
            for (int r = 0; r < root; r++) { so += totals[r]; lo += nbs[r]; }
            if (totals[root]) HIPCHK(rt, hipMemcpyAsync(d_out + so, src_out[root], (size_t)totals[root], hipMemcpyDeviceToDevice, rt->stream));
            if (nbs[root]) HIPCHK(rt, hipMemcpyAsync(d_block_lens + lo, src_lens[root], nbs[root] * 4, hipMemcpyDeviceToDevice, rt->stream));
        }
        int gs = rc_api->GroupStart();
        const bool opened = gs == w3rccl::kSuccess;
        uint64_t so = 0; size_t lo = 0;
        for (int r = 0; r < n_ctx; r++) {
            w3_ctx *c = ctxs[r];
            if (r != root && nbs[r] && gs == w3rccl::kSuccess) {
                (void)hipSetDevice(c->device);
                // seven peers each have their own xGMI link to the root: the transfers of one group run concurrently
                gs = rc_api->Send(src_out[r], (size_t)totals[r], w3rccl::kUint8, root, cm->comms[r], c->stream);
                if (gs == w3rccl::kSuccess) gs = rc_api->Send(src_lens[r], nbs[r] * 4, w3rccl::kUint8, root, cm->comms[r], c->stream);
                (void)hipSetDevice(rt->device);
                if (gs == w3rccl::kSuccess) gs = rc_api->Recv(d_out + so, (size_t)totals[r], w3rccl::kUint8, r, cm->comms[root], rt->stream);
                if (gs == w3rccl::kSuccess) gs = rc_api->Recv(d_block_lens + lo, nbs[r] * 4, w3rccl::kUint8, r, cm->comms[root], rt->stream);
            }
            so += totals[r]; lo += nbs[r];
        }
        const int ge = opened ? rc_api->GroupEnd() : w3rccl::kSuccess;
        if (gs != w3rccl::kSuccess || ge != w3rccl::kSuccess) { ctxs[0]->err = std::string("RCCL gather: ") + rc_api->GetErrorString(gs != w3rccl::kSuccess ? gs : ge); return W3_E_HIP; }
        for (int r = 0; r < n_ctx; r++) {
            HIPCHK(ctxs[r], hipSetDevice(ctxs[r]->device));
            HIPCHK(ctxs[r], hipStreamSynchronize(ctxs[r]->stream));
        }
    } else {
        // device copies (same device: D2D; other devices: peer copies over xGMI / PCIe, no RCCL needed)
        uint64_t so = 0; size_t lo = 0;
        for (int r = 0; r < n_ctx; r++) {
            w3_ctx *c = ctxs[r];
            if (nbs[r]) {
                if (c->device == rt->device) {
                    HIPCHK(rt, hipMemcpyAsync(d_out + so, src_out[r], (size_t)totals[r], hipMemcpyDeviceToDevice, rt->stream));
                    HIPCHK(rt, hipMemcpyAsync(d_block_lens + lo, src_lens[r], nbs[r] * 4, hipMemcpyDeviceToDevice, rt->stream));
                } else {
                    HIPCHK(rt, hipMemcpyPeerAsync(d_out + so, rt->device, src_out[r], c->device, (size_t)totals[r], rt->stream));
                    HIPCHK(rt, hipMemcpyPeerAsync(d_block_lens + lo, rt->device, src_lens[r], c->device, nbs[r] * 4, rt->stream));
                }
            }
            so += totals[r]; lo += nbs[r];
        }
        HIPCHK(rt, hipStreamSynchronize(rt->stream));
    }
    return W3_OK;
}

extern "C" int w3_rccl_library(const char *path) {
    std::lock_guard<std::mutex> lk(g_comm_mu);
    if (w3rccl::resolved()) return W3_E_INVALID;   // (the library is resolved once per process, at the first gather or status call)
    w3rccl::library_override() = path ? path : "";
    return W3_OK;
}

extern "C" int w3_rccl_status(char *msg, size_t cap) {
    w3rccl::Api *r;
    { std::lock_guard<std::mutex> lk(g_comm_mu); r = w3rccl::api(); }
    if (msg && cap) { snprintf(msg, cap, "%s", r->error.empty() ? "RCCL resolved" : r->error.c_str()); }
    return r->error.empty() ? W3_OK : W3_E_HIP;
}

extern "C" int w3_encode_blocks_sharded_device(w3_ctx *const *ctxs, int n_ctx, const w3_model_spec *spec, const uint8_t *const *d_in, const size_t *n,
                                               size_t block_size, int root, uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens,
                                               uint64_t *totals, int transport) {
    if (!ctxs || n_ctx <= 0 || n_ctx > 64 || !d_in || !n || !totals || root < 0 || root >= n_ctx) return W3_E_INVALID;
    if (transport < W3_GATHER_AUTO || transport > W3_GATHER_PEER_COPY) return W3_E_INVALID;
    std::vector<int> devs(n_ctx);
    bool distinct = true;
    size_t nb_total = 0;
    for (int r = 0; r < n_ctx; r++) {
        if (!ctxs[r]) return W3_E_INVALID;
        for (int q = 0; q < r; q++) {
            if (ctxs[q] == ctxs[r]) { ctxs[0]->err = "the same context appears twice in ctxs[] (a context is not thread-safe)"; return W3_E_INVALID; }
            distinct &= ctxs[q]->device != ctxs[r]->device;
        }
        devs[r] = ctxs[r]->device;
        totals[r] = 0;
        int rc = check_args(ctxs[r], n[r], block_size);
        if (rc) return rc;
        if (n[r] && !d_in[r]) return W3_E_INVALID;
        if (r + 1 < n_ctx && n[r] % block_size) { ctxs[0]->err = "every shard but the last must be a whole number of blocks (w3_shard_range)"; return W3_E_INVALID; }
        if ((rc = jobs_idle(ctxs[r]))) return rc;
        nb_total += (n[r] + block_size - 1) / block_size;
    }
    if (nb_total == 0) return w3_spec_validate(spec);
    if (!d_out || !d_block_lens) return W3_E_INVALID;
    // RCCL needs one device per rank (ncclCommInitAll refuses a device twice): contexts that share a device — how the path is
    // rehearsed on a 1-GPU box — gather with device copies instead
    const bool use_rccl = transport == W3_GATHER_RCCL || (transport == W3_GATHER_AUTO && distinct && n_ctx > 1);
    if (use_rccl && !distinct) { ctxs[0]->err = "W3_GATHER_RCCL needs one device per context"; return W3_E_INVALID; }
    ShardComms *cm = nullptr;
    if (use_rccl && !(cm = shard_comms(devs, ctxs[0]->err))) return W3_E_HIP;

    // 1. every shard on its own device and host thread, into its context's staging buffers (io_out, lens, total)
    std::vector<int> rcs(n_ctx, W3_OK);
    std::vector<size_t> nbs(n_ctx, 0);
    {
        std::vector<std::thread> th;
        for (int r = 0; r < n_ctx; r++) {
            nbs[r] = (n[r] + block_size - 1) / block_size;
            if (!nbs[r]) continue;
            th.emplace_back([&, r]() {
                w3_ctx *c = ctxs[r];
                auto body = [&]() -> int {
                    HIPCHK(c, hipSetDevice(c->device));
                    size_t cap = n[r] + n[r] / 4 + 64 * nbs[r] + 1024;   // realistic bound; grown to the reported need on W3_E_NOSPACE
                    for (int attempt = 0; attempt < 2; attempt++) {
                        ENSURE(c, c->io_out, cap);
                        ENSURE(c, c->lens, nbs[r] * 4);
                        ENSURE(c, c->total, 8);
                        int rc = encode_core(c, c->jobs[0], spec, d_in[r], n[r], block_size, (uint8_t *)c->io_out.p, cap, (uint32_t *)c->lens.p, (uint64_t *)c->total.p, nullptr);
                        uint64_t t = 0;
                        if (rc == W3_OK || rc == W3_E_NOSPACE) HIPCHK(c, hipMemcpy(&t, c->total.p, 8, hipMemcpyDeviceToHost));
                        totals[r] = t;
                        if (rc != W3_E_NOSPACE || t <= cap) return rc;
                        cap = (size_t)t;
                    }
                    return W3_E_NOSPACE;
                };
                rcs[r] = body();
            });
        }
        for (auto &t : th) t.join();
    }
    for (int r = 0; r < n_ctx; r++)
        if (rcs[r]) { if (r) ctxs[0]->err = "shard " + std::to_string(r) + ": " + (ctxs[r]->err.empty() ? w3_strerror(rcs[r]) : ctxs[r]->err); return rcs[r]; }

    std::vector<void *> so(n_ctx), sl(n_ctx), st(n_ctx);
    for (int r = 0; r < n_ctx; r++) {
        w3_ctx *c = ctxs[r];
        HIPCHK(c, hipSetDevice(c->device));
        ENSURE(c, c->total, 8);
        so[r] = c->io_out.p; sl[r] = c->lens.p; st[r] = c->total.p;
    }
    return shard_gather(ctxs, n_ctx, root, cm, so.data(), sl.data(), st.data(), nbs, totals, d_out, out_cap, d_block_lens);
}

// ---------------------------------------------------------------------------
// The sharded encode as a STREAM of steps (ABI v8): every context keeps w3_encode_max_in_flight calls in flight on its device
// (w3_encode_submit), and a step's packed streams are gathered on the root when the step is waited for — the exchange step of step k
// runs on the contexts' own streams while the devices are already coding step k+1.  What bench.py --gpus N does through
// torch.distributed (one process per GPU), for a host that is ONE process.
// ---------------------------------------------------------------------------
static int sharded_args(w3_ctx *const *ctxs, int n_ctx, std::vector<int> &devs, bool &distinct) {
    if (!ctxs || n_ctx <= 0 || n_ctx > 64) return W3_E_INVALID;
    devs.assign(n_ctx, 0);
    distinct = true;
    for (int r = 0; r < n_ctx; r++) {
        if (!ctxs[r]) return W3_E_INVALID;
        for (int q = 0; q < r; q++) {
            if (ctxs[q] == ctxs[r]) { ctxs[0]->err = "the same context appears twice in ctxs[] (a context is not thread-safe)"; return W3_E_INVALID; }
            distinct &= ctxs[q]->device != ctxs[r]->device;
        }
        devs[r] = ctxs[r]->device;
    }
    return W3_OK;
}

extern "C" int w3_encode_sharded_max_in_flight(const w3_model_spec *spec, const size_t *n, int n_ctx, size_t block_size) {
    if (!n || n_ctx <= 0 || !block_size) return 0;
    int depth = W3_MAX_JOBS;
    for (int r = 0; r < n_ctx; r++)
        if (n[r]) depth = std::min(depth, w3_encode_max_in_flight(spec, n[r], block_size));
    return depth;
}

extern "C" int w3_encode_sharded_submit(w3_ctx *const *ctxs, int n_ctx, const w3_model_spec *spec, const uint8_t *const *d_in, const size_t *n,
                                        size_t block_size, int *sjob) {
    if (!sjob || !d_in || !n) return W3_E_INVALID;
    *sjob = -1;
    std::vector<int> devs;
    bool distinct;
    int rc = sharded_args(ctxs, n_ctx, devs, distinct);
    if (rc) return rc;
    ParsedSpec ps;
    if ((rc = parse_spec(spec, ps))) { ctxs[0]->err = "malformed model spec"; return rc; }
    size_t nb_total = 0;
    for (int r = 0; r < n_ctx; r++) {
        if ((rc = check_args(ctxs[r], n[r], block_size))) return rc;
        if (n[r] && !d_in[r]) return W3_E_INVALID;
        if (r + 1 < n_ctx && n[r] % block_size) { ctxs[0]->err = "every shard but the last must be a whole number of blocks (w3_shard_range)"; return W3_E_INVALID; }
        const size_t nb = (n[r] + block_size - 1) / block_size;
        nb_total += nb;
        // (a shard that w3_encode_submit runs synchronously — a ragged tail below 8 bytes, a lane-per-block spec — is coded inside this
        // call, one context after the other: correct, but such specs are better served by the one-shot form, which codes the shards from
        // one host thread each)
        for (const auto &h : ctxs[r]->hj)
            if (h.state != 0) { ctxs[0]->err = "host-buffer jobs are in flight on a context"; return W3_E_INVALID; }
    }
    if (nb_total == 0) { ctxs[0]->err = "nothing to encode"; return W3_E_INVALID; }
    // the same slot on every context; as many steps in flight as the smallest w3_encode_max_in_flight among the shards
    int busy[W3_MAX_JOBS] = {};   // (a slot is taken while any context holds a shard in it)
    for (int k = 0; k < W3_MAX_JOBS; k++)
        for (int r = 0; r < n_ctx; r++) busy[k] |= ctxs[r]->ss[k].state;
    const int depth = w3_encode_sharded_max_in_flight(spec, n, n_ctx, block_size);
    const SlotPick pick = pick_slot(busy, W3_MAX_JOBS, 0, depth);   // (the first free slot)
    const int slot = pick.slot;
    if (slot < 0) {
        ctxs[0]->err = std::to_string(pick.in_flight) + " sharded steps are in flight already (at most " + std::to_string(depth) + " for shards of this size): w3_encode_sharded_wait the oldest one first";
        return W3_E_INVALID;
    }
    for (int r = 0; r < n_ctx; r++) {
        w3_ctx *c = ctxs[r];
        w3_ctx::ShardSlot &x = c->ss[slot];
        auto body = [&]() -> int {
            HIPCHK(c, hipSetDevice(c->device));
            x.nb = (n[r] + block_size - 1) / block_size; x.djob = -1;
            x.call.keep(spec, ps, d_in[r], n[r], block_size);
            ENSURE(c, x.total, 8);
            if (!x.nb) { HIPCHK(c, hipMemsetAsync(x.total.p, 0, 8, c->stream)); return W3_OK; }
            x.cap = n[r] + n[r] / 4 + 64 * x.nb + 1024;   // realistic bound; a shard beyond it is redone with the room it asks for (the wait)
            ENSURE(c, x.out, x.cap);
            ENSURE(c, x.lens, x.nb * 4);
            return w3_encode_submit(c, &x.call.spec, d_in[r], n[r], block_size, (uint8_t *)x.out.p, x.cap, (uint32_t *)x.lens.p, (uint64_t *)x.total.p, nullptr, &x.djob);
        };
        rc = body();
        if (rc) {   // leave nothing in flight behind an error: the shards submitted so far are completed and dropped
            if (r) ctxs[0]->err = "shard " + std::to_string(r) + ": " + (c->err.empty() ? w3_strerror(rc) : c->err);
            for (int q = 0; q < r; q++) {
                w3_ctx::ShardSlot &y = ctxs[q]->ss[slot];
                if (y.djob >= 0) (void)w3_encode_wait(ctxs[q], y.djob);
                y.state = 0; y.djob = -1;
            }
            return rc;
        }
        x.state = 1;
    }
    *sjob = slot;
    return W3_OK;
}

extern "C" int w3_encode_sharded_wait(w3_ctx *const *ctxs, int n_ctx, int sjob, int root, uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens,
                                      uint64_t *totals, int transport) {
    if (!totals || sjob < 0 || sjob >= W3_MAX_JOBS || root < 0 || root >= n_ctx) return W3_E_INVALID;
    if (transport < W3_GATHER_AUTO || transport > W3_GATHER_PEER_COPY) return W3_E_INVALID;
    std::vector<int> devs;
    bool distinct;
    int rc = sharded_args(ctxs, n_ctx, devs, distinct);
    if (rc) return rc;
    for (int r = 0; r < n_ctx; r++)
        if (ctxs[r]->ss[sjob].state != 1) { ctxs[0]->err = "no such sharded step in flight"; return W3_E_INVALID; }
    if (!d_out || !d_block_lens) return W3_E_INVALID;
    const bool use_rccl = transport == W3_GATHER_RCCL || (transport == W3_GATHER_AUTO && distinct && n_ctx > 1);
    if (use_rccl && !distinct) { ctxs[0]->err = "W3_GATHER_RCCL needs one device per context"; return W3_E_INVALID; }
    // 1. the shards' encodes (the devices run them concurrently; the waits only read pinned status words)
    std::vector<size_t> nbs(n_ctx, 0);
    int first_rc = W3_OK;
    for (int r = 0; r < n_ctx; r++) {
        w3_ctx *c = ctxs[r];
        w3_ctx::ShardSlot &x = c->ss[sjob];
        nbs[r] = x.nb;
        totals[r] = 0;
        auto body = [&]() -> int {
            if (x.djob < 0) return W3_OK;
            int rc1 = w3_encode_wait(c, x.djob);
            uint64_t t = 0;
            const Job &ds = c->jobs[x.djob];
            if (rc1 == W3_OK || rc1 == W3_E_NOSPACE) {
                if (ds.total_valid) t = ds.total_out;
                else { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipMemcpy(&t, x.total.p, 8, hipMemcpyDeviceToHost)); }
            }
            if (rc1 == W3_E_NOSPACE && t > x.cap) {
                rc1 = redo_with_room(c, x.call, x.djob, ds.call.vcall, x.out, x.cap, t, x.lens, x.total);
                if (rc1 == W3_OK) HIPCHK(c, hipMemcpy(&t, x.total.p, 8, hipMemcpyDeviceToHost));
            }
            totals[r] = t;
            return rc1;
        };
        const int rc1 = body();
        if (rc1 && first_rc == W3_OK) { first_rc = rc1; if (r) ctxs[0]->err = "shard " + std::to_string(r) + ": " + (c->err.empty() ? w3_strerror(rc1) : c->err); }
    }
    // 2. the exchange step
    int grc = first_rc;
    if (grc == W3_OK) {
        ShardComms *cm = nullptr;
        if (use_rccl && !(cm = shard_comms(devs, ctxs[0]->err))) grc = W3_E_HIP;
        if (grc == W3_OK) {
            std::vector<void *> so(n_ctx), sl(n_ctx), st(n_ctx);
            for (int r = 0; r < n_ctx; r++) { w3_ctx::ShardSlot &x = ctxs[r]->ss[sjob]; so[r] = x.out.p; sl[r] = x.lens.p; st[r] = x.total.p; }
            grc = shard_gather(ctxs, n_ctx, root, cm, so.data(), sl.data(), st.data(), nbs, totals, d_out, out_cap, d_block_lens);
        }
    }
    for (int r = 0; r < n_ctx; r++) { ctxs[r]->ss[sjob].state = 0; ctxs[r]->ss[sjob].djob = -1; }
    return grc;
}

// ---------------------------------------------------------------------------
// reference container: b"w30i" + u64 BE len + one stream  (main.rs:14-15, 89-144)
// ---------------------------------------------------------------------------
extern "C" int w3_compress_stream(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, uint8_t *out, size_t out_cap,
                                  size_t *out_len) {
    if (!ctx || !out_len) return W3_E_INVALID;
    *out_len = 0;
    // One stream is one serial chain = ONE GPU lane (~260 ns per bit-step: 2^28 bytes take ~10 minutes); larger inputs belong in the block
    // container, which is what the device is for — the reference's format has no blocks to code in parallel.
    if (n > (1u << 28)) { ctx->err = "the w30i single-stream container is limited to 2^28 bytes on the device (one serial chain = one GPU lane): use the block container (w3_encode_blocks; tools/w3cli without W3_CONTAINER=w30i) for larger inputs"; return W3_E_UNSUPPORTED; }
    int rc = w3_spec_validate(spec);
    if (rc) return rc;
    uint8_t hdr[12] = {'w', '3', '0', 'i'};
    for (int i = 0; i < 8; i++) hdr[4 + i] = (uint8_t)((uint64_t)n >> (8 * (7 - i)));
    size_t body = 0;
    if (n == 0) {
        // empty file: the coder still flushes x2 = 0xFFFFFFFF -> one 0xFF byte (io.rs:91-100)
        *out_len = 13;
        if (out_cap < 13 || !out) return W3_E_NOSPACE;
        memcpy(out, hdr, 12);
        out[12] = 0xFF;
        return W3_OK;
    }
    uint32_t blen = 0;
    rc = w3_encode_blocks(ctx, spec, in, n, n, out_cap > 12 && out ? out + 12 : nullptr, out_cap > 12 ? out_cap - 12 : 0, &body, &blen);
    *out_len = body + 12;
    if (rc) return rc;
    memcpy(out, hdr, 12);
    return W3_OK;
}

extern "C" int w3_decompress_stream(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t in_len, uint8_t *out,
                                    size_t out_cap, size_t *out_len) {
    if (!ctx || !in || !out_len) return W3_E_INVALID;
    *out_len = 0;
    if (in_len < 12) { ctx->err = "truncated header"; return W3_E_FORMAT; }
    if (memcmp(in, "w30i", 4) != 0) { ctx->err = "Magic numbers don't match up"; return W3_E_FORMAT; }
    uint64_t len = 0;
    for (int i = 0; i < 8; i++) len = (len << 8) | in[4 + i];
    *out_len = (size_t)len;
    if (len == 0) return w3_spec_validate(spec);
    if (len > (1u << 28)) { ctx->err = "the w30i single-stream container is limited to 2^28 bytes on the device (one serial chain = one GPU lane); larger inputs use the block container (w3_decode_blocks)"; return W3_E_UNSUPPORTED; }
    if (len > out_cap || !out) return W3_E_NOSPACE;
    uint32_t blen = (uint32_t)(in_len - 12);
    uint8_t zero = 0;
    const uint8_t *body = blen ? in + 12 : &zero;  // ACReader pads with zeros past EOF (io.rs:23-26)
    return w3_decode_blocks(ctx, spec, body, blen, &blen, 1, (size_t)len, len, out);
}

// ---------------------------------------------------------------------------
// StationaryModel::new (models/ac_hash/stationary.rs:14-34): constructor-time
// table prep on the host (8 Counters, one per bit position, index 0 = MSB).
// ---------------------------------------------------------------------------
extern "C" int w3_stationary_table(const uint8_t *buf, size_t n, uint16_t table[8]) {
    if ((!buf && n) || !table) return W3_E_INVALID;
    uint32_t c0[8] = {0}, c1[8] = {0};
    for (size_t k = 0; k < n; k++) {
        for (int i = 0; i < 8; i++) {
            uint32_t bit = (buf[k] >> (7 - i)) & 1u;
            uint32_t &c = bit ? c1[i] : c0[i];
            if (++c == 0xFFFFu) {  // Counter::update halves BOTH counts (counter.rs:22-25)
                c0[i] = (c0[i] >> 1) + (c0[i] & 1u);
                c1[i] = (c1[i] >> 1) + (c1[i] & 1u);
            }
        }
    }
    for (int i = 0; i < 8; i++) {
        uint64_t p = (1ull << 17) * ((uint64_t)c1[i] + 1) / ((uint64_t)c0[i] + c1[i] + 2);
        table[i] = (uint16_t)((p >> 1) + (p & 1));
    }
    return W3_OK;
}

// ---------------------------------------------------------------------------
// OrderN(bits, align) parameter sweep, configurations x blocks in one launch (w3_sweep.h; bin/ordern/main.rs:9-80)
// ---------------------------------------------------------------------------
extern "C" int w3_sweep_ordern_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, const uint8_t *bits, const uint8_t *aligns,
                                      size_t ncfg, uint32_t *block_bits) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;
    const uint32_t nb = (uint32_t)((n + block_size - 1) / block_size);
    if (nb == 0 || ncfg == 0) return W3_OK;
    if (!d_in || !bits || !aligns || !block_bits || ncfg > 4096) return W3_E_INVALID;
    for (size_t c = 0; c < ncfg; c++)   // OrderN::new allocates 1 << bits counters; masks are u32 (ordern.rs:35-43)
        if (bits[c] < 1 || bits[c] > 32 || aligns[c] > 7 || aligns[c] > bits[c] || (int)bits[c] - (int)aligns[c] > 31) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<SweepCfg> cfg(ncfg);
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = sweep_budget(free_b, ctx->tables.cap);
    ENSURE(ctx, ctx->sweep, ncfg * sizeof(SweepCfg) + (size_t)ncfg * nb * 4);
    SweepCfg *d_cfg = (SweepCfg *)ctx->sweep.p;
    uint32_t *d_bits = (uint32_t *)((uint8_t *)ctx->sweep.p + ncfg * sizeof(SweepCfg));
    SweepArgs a;
    memset(&a, 0, sizeof a);
    a.in = d_in; a.n = n; a.block_size = (uint32_t)block_size; a.nblocks = nb; a.waves_per_cfg = (nb + 63) / 64; a.ncfg = (uint32_t)ncfg;
    a.cfg = d_cfg; a.out_bits = d_bits;
    size_t c0 = 0;
    while (c0 < ncfg) {   // as many configurations per launch as their tables fit the budget
        uint64_t used = 0;
        size_t c1 = c0;
        for (; c1 < ncfg; c1++) {
            const CounterTable t = counter_table(bits[c1], (uint64_t)block_size * 8);
            const uint64_t stride = t.use_hash ? t.hash_bytes : std::max<uint64_t>(t.direct_bytes, 16);
            if (c1 > c0 && used + stride * nb > budget) break;
            SweepCfg &cf = cfg[c1];
            cf.bits = bits[c1]; cf.align = aligns[c1]; cf.use_hash = t.use_hash; cf.pad = 0;
            cf.hash_mask = (uint32_t)(t.slots - 1); cf.hist_mask = (uint32_t)((1ull << (bits[c1] - aligns[c1])) - 1ull);
            cf.base = used; cf.stride = stride;
            used += stride * nb;
        }
        if (used > (uint64_t)(free_b + ctx->tables.cap)) { ctx->err = "sweep tables of one configuration do not fit the device"; return W3_E_NOMEM; }
        ENSURE(ctx, ctx->tables, (size_t)used);
        HIPCHK(ctx, hipMemsetAsync(ctx->tables.p, 0, (size_t)used, s));
        HIPCHK(ctx, hipMemcpyAsync(d_cfg + c0, cfg.data() + c0, (c1 - c0) * sizeof(SweepCfg), hipMemcpyHostToDevice, s));
        a.tables = (uint8_t *)ctx->tables.p; a.first_cfg = (uint32_t)c0;
        hipLaunchKernelGGL(k_sweep_ordern, dim3((unsigned)((c1 - c0) * a.waves_per_cfg)), dim3(64), 0, s, a);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(s));   // (cfg is host memory reused by the next batch; the tables are re-zeroed)
        c0 = c1;
    }
    HIPCHK(ctx, hipMemcpy(block_bits, d_bits, (size_t)ncfg * nb * 4, hipMemcpyDeviceToHost));
    return W3_OK;
}

extern "C" int w3_sweep_ordern(w3_ctx *ctx, const uint8_t *in, size_t n, size_t block_size, const uint8_t *bits, const uint8_t *aligns,
                               size_t ncfg, uint32_t *block_bits) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;
    if (n == 0 || ncfg == 0) return W3_OK;
    if (!in) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->io_in, n);
    HIPCHK(ctx, hipMemcpy(ctx->io_in.p, in, n, hipMemcpyHostToDevice));
    return w3_sweep_ordern_device(ctx, (const uint8_t *)ctx->io_in.p, n, block_size, bits, aligns, ncfg, block_bits);
}

// ---------------------------------------------------------------------------
// AC over Huffman (w3_aoh.h; bin/ac-over-huffman/main.rs:46-89): OrderN(ctx_bits, 0) over the bits of the input's canonical Huffman
// codes.  One fused lane-per-block kernel for the counting sink, the sweep, encode and decode; encode and the counting sink of one
// configuration also in the two-phase form (W3_OPT_PATH; aoh_twophase_run).
// ---------------------------------------------------------------------------
extern "C" int w3_huff_code_table(const uint8_t *buf, size_t n, uint8_t huffman_size, w3_huff_code *out) {
    if ((!buf && n) || !out) return W3_E_INVALID;
    uint64_t c64[256] = {0};
    for (size_t i = 0; i < n; i++) c64[buf[i]]++;                      // histogram (helpers.rs:30-36) of the WHOLE buffer (:74)
    return w3_huff_code_from_counts(c64, huffman_size, out);
}

// the reference counts in u32 (helpers.rs:30-36): W3_E_UNSUPPORTED for a count it could not hold
static int counts_to_u32(const uint64_t c64[256], uint32_t counts[256]) {
    for (int s = 0; s < 256; s++) {
        if (c64[s] > 0xFFFFFFFFull) return W3_E_UNSUPPORTED;
        counts[s] = (uint32_t)c64[s];
    }
    return W3_OK;
}

// ... from the histogram alone (w3_histogram / w3_histogram_device): the one builder of the code
extern "C" int w3_huff_code_from_counts(const uint64_t c64[256], uint8_t huffman_size, w3_huff_code *out) {
    if (!c64 || !out) return W3_E_INVALID;
    uint32_t counts[256];
    if (const int rc = counts_to_u32(c64, counts)) return rc;
    uint8_t lens[256];
    if (!w3huff::code_lengths(counts, 256, huffman_size, lens)) return W3_E_INVALID;   // package_merge's three asserts (:75)
    for (int s = 0; s < 256; s++)
        if (lens[s] > 16) return W3_E_INVALID;                          // codes are u16 (package_merge.rs:87)
    w3aoh::canonical(lens, out);                                        // :76
    return W3_OK;
}

extern "C" size_t w3_aoh_max_compressed_size(size_t n, size_t block_size, const w3_huff_code *code) {
    if (block_size == 0 || !w3aoh::valid(code)) return 0;
    const size_t nb = (n + block_size - 1) / block_size;
    return 2 * (size_t)w3aoh::max_len(code) * n + 8 * nb + 8;           // 16 output bits per coded bit, flush bytes per block
}

// argument checks shared by the family; *max_len_out = the longest code of the (first) table
static int aoh_check(w3_ctx *ctx, const w3_huff_code *codes, size_t n_codes, const uint8_t *ctx_bits, size_t ncfg, size_t n, size_t block_size,
                     bool one_device) {
    int rc = check_args(ctx, n, block_size, one_device);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;
    if (!codes || !ctx_bits) { ctx->err = "null code table or ctx_bits"; return W3_E_INVALID; }
    for (size_t k = 0; k < n_codes; k++) {
        if (!w3aoh::valid(codes + k)) { ctx->err = "code table " + std::to_string(k) + " is not a canonical code (w3hip.h: Validation)"; return W3_E_INVALID; }
        if ((uint64_t)block_size * w3aoh::max_len(codes + k) >= (1ull << 32)) { ctx->err = "block_size x max code length must be below 2^32"; return W3_E_INVALID; }
    }
    for (size_t c = 0; c < ncfg; c++)   // OrderN::new(ctx_bits, 0): masks are u32, bits - align <= 31 (ordern.rs:35-43)
        if (ctx_bits[c] < 1 || ctx_bits[c] > 31) { ctx->err = "ctx_bits must be in 1..31"; return W3_E_INVALID; }
    return W3_OK;
}

struct AohPrep {
    AohDev *d_codes = nullptr; AohCfg *d_cfg = nullptr;
    uint32_t *d_L = nullptr, *d_max = nullptr, *d_flags = nullptr;
    std::vector<uint32_t> max_l, flags;   // per code table: the call's largest L_b; 1 = the input holds a byte with len 0
};

// Code tables to the device; with d_in, the length pre-pass (k_aoh_lens).  Synchronises the stream.
static int aoh_prepare(w3_ctx *ctx, hipStream_t s, const w3_huff_code *codes, size_t n_codes, size_t ncfg, uint32_t nb, const uint8_t *d_in, size_t n,
                       size_t block_size, AohPrep &P) {
    auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    const size_t o_cfg = up16(n_codes * sizeof(AohDev)), o_L = o_cfg + up16(ncfg * sizeof(AohCfg)), o_max = o_L + up16(n_codes * (size_t)nb * 4),
                 o_flags = o_max + up16(n_codes * 4), total = o_flags + up16(n_codes * 4);
    ENSURE(ctx, ctx->aoh, total);
    uint8_t *base = (uint8_t *)ctx->aoh.p;
    P.d_codes = (AohDev *)base; P.d_cfg = (AohCfg *)(base + o_cfg); P.d_L = (uint32_t *)(base + o_L);
    P.d_max = (uint32_t *)(base + o_max); P.d_flags = (uint32_t *)(base + o_flags);
    std::vector<AohDev> h(n_codes);
    for (size_t k = 0; k < n_codes; k++) w3aoh::to_device_form(codes + k, &h[k]);
    HIPCHK(ctx, hipMemcpyAsync(P.d_codes, h.data(), n_codes * sizeof(AohDev), hipMemcpyHostToDevice, s));
    P.max_l.assign(n_codes, 0); P.flags.assign(n_codes, 0);
    if (d_in) {
        HIPCHK(ctx, hipMemsetAsync(P.d_max, 0, total - o_max, s));
        hipLaunchKernelGGL(k_aoh_lens, dim3(std::min<uint32_t>(nb, 4096u), (unsigned)n_codes), dim3(64), 0, s, d_in, (uint64_t)n, (uint32_t)block_size, nb,
                           (const AohDev *)P.d_codes, P.d_L, P.d_max, P.d_flags);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(P.max_l.data(), P.d_max, n_codes * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(P.flags.data(), P.d_flags, n_codes * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));   // (h is host memory of this frame)
    return W3_OK;
}

// The sweep family's workspace in ctx->tables: plan(budget) lays a call out within `budget` bytes and returns the bytes it needs (0:
// it does not fit; plan has set ctx->err).  One hipMalloc of that size can fail although hipMemGetInfo calls the memory free
// (table_budget): the plan is then made again with half the budget.
template <class Plan>
static int ensure_sweep_tables(w3_ctx *ctx, Plan &&plan) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    for (uint64_t budget = sweep_budget(free_b, ctx->tables.cap);; budget /= 2) {
        const uint64_t need = plan(budget);
        if (!need) return W3_E_NOMEM;
        const int rc = ensure(ctx, ctx->tables, (size_t)need);
        if (rc != W3_E_NOMEM || budget < (1ull << 20)) return rc;
    }
}

// Launch k_aoh<MODE> for configurations cfg[] (ctx_bits and code_idx set) x blocks [0, nb): per lane a Counter table in the form of
// counter_table(ctx_bits, steps[c]) (steps[c]: the most steps one lane of configuration c can take), in the launches of
// plan_cfg_batches (w3_tables_plan.h) under the budget of ensure_sweep_tables.  Tables are zero-filled per batch.
// max_lanes (the decoders' job calls under W3_OPT_AOH_BATCH_BLOCKS; 0 = no cap): most lanes per batch.
template <int MODE>
static int aoh_launch(w3_ctx *ctx, hipStream_t s, AohArgs a, AohPrep &P, std::vector<AohCfg> &cfg, const std::vector<uint64_t> &steps, uint32_t nb,
                      uint32_t max_lanes = 0) {
    const size_t ncfg = cfg.size();
    std::vector<uint64_t> strides(ncfg), base(ncfg);
    for (size_t c = 0; c < ncfg; c++) {
        const CounterTable t = counter_table(cfg[c].ctx_bits, steps[c]);
        AohCfg &cf = cfg[c];
        cf.use_hash = t.use_hash; cf.pad = 0;
        cf.hash_mask = (uint32_t)(t.slots - 1); cf.ctx_mask = (uint32_t)((1ull << cf.ctx_bits) - 1ull);
        cf.stride = strides[c] = t.use_hash ? t.hash_bytes : std::max<uint64_t>(t.direct_bytes, 16);
    }
    std::vector<CfgBatch> plan;
    const int rc = ensure_sweep_tables(ctx, [&](uint64_t budget) {
        uint64_t need = 0;
        if (!plan_cfg_batches(strides.data(), ncfg, nb, budget, max_lanes, plan, base.data(), need)) { ctx->err = "the Counter table of one lane does not fit the device budget"; return (uint64_t)0; }
        return need;
    });
    if (rc) return rc;
    for (size_t c = 0; c < ncfg; c++) cfg[c].base = base[c];
    HIPCHK(ctx, hipMemcpy(P.d_cfg, cfg.data(), ncfg * sizeof(AohCfg), hipMemcpyHostToDevice));
    a.cfg = P.d_cfg; a.codes = P.d_codes; a.tables = (uint8_t *)ctx->tables.p; a.nblocks = nb;
    for (const CfgBatch &bt : plan) {
        HIPCHK(ctx, hipMemsetAsync(ctx->tables.p, 0, (size_t)bt.used, s));
        a.first_cfg = (uint32_t)bt.c0; a.first_block = bt.first_block; a.n_lanes = bt.n_lanes; a.waves_per_cfg = (bt.n_lanes + 63) / 64;
        hipLaunchKernelGGL(k_aoh<MODE>, dim3((unsigned)((bt.c1 - bt.c0) * a.waves_per_cfg)), dim3(64), 0, s, a);
        HIPCHK(ctx, hipGetLastError());
    }
    return W3_OK;
}

// The Counter table of one resident wavefront of k_aoh_predict: direct [2^ctx_bits] where that is no larger than the exact map of
// k_predict_wave's form (twice as many slots as the call's longest block has steps, and ctx 0's own slot behind them).
struct AohWaveTable { bool use_hash; uint64_t slots, stride; };
static AohWaveTable aoh_wave_table(uint8_t ctx_bits, uint64_t max_l) {
    const CounterTable c = counter_table(ctx_bits, max_l);
    return AohWaveTable{c.use_hash, c.slots, c.use_hash ? c.hash_bytes + 16 : std::max<uint64_t>(c.direct_bytes, 16)};
}

// which form a call takes (W3_OPT_PATH; W3_PATH_AUTO by the measured rule of w3_aoh.h)
static bool aoh_takes_twophase(const w3_ctx *ctx, uint32_t nb, uint8_t ctx_bits, uint64_t max_l) {
    if (ctx->opt_path != W3_PATH_AUTO) return ctx->opt_path == W3_PATH_TWOPHASE;
    return aoh_auto_twophase(nb, ctx_bits, aoh_wave_table(ctx_bits, max_l).use_hash);
}

// The two-phase form (w3_aoh.h) of encode (STATS = false: into the stripes, as aoh_launch<AOH_ENCODE>) and of the counting sink, one
// configuration: per batch of whole blocks (w3_aoh_plan.h) k_aoh_pack, k_aoh_predict, k_aoh_coder.  ONE allocation (ctx->tables) holds
// the plan's offsets, the Counter tables of the resident wavefronts, P and the strings; the budget is ensure_sweep_tables', a call whose
// workspace exceeds it goes in batches (W3_OPT_AOH_BATCH_BLOCKS: the tests' cap on a batch).  With W3_OPT_TIMING the phases' times
// are added to ctx->timing batch by batch.
template <bool STATS>
static int aoh_twophase_run(w3_ctx *ctx, hipStream_t s, AohTwoArgs a, AohPrep &P, uint8_t ctx_bits, uint32_t nb) {
    std::vector<uint32_t> L(nb);
    HIPCHK(ctx, hipMemcpyAsync(L.data(), P.d_L, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    const AohWaveTable tk = aoh_wave_table(ctx_bits, P.max_l[0]);
    auto up256 = [](uint64_t v) { return (v + 255) / 256 * 256; };
    const uint64_t meta = up256((uint64_t)nb * 16);
    uint64_t resident = 256 * 32;
    {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_aoh_predict, 64, 0) == hipSuccess && per_cu > 0 &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0)
            resident = (uint64_t)per_cu * (uint64_t)cus;
        else (void)hipGetLastError();
    }
    AohPlan plan;
    uint64_t waves = 0, o_P = 0, o_str = 0;
    const int rc = ensure_sweep_tables(ctx, [&](uint64_t budget) -> uint64_t {
        // latency-bound: as many wavefronts as the chip holds of this kernel (more would queue behind them with tables of their own), their
        // tables within half the budget
        waves = std::min<uint64_t>(std::min<uint64_t>(nb, resident), budget / 2 / tk.stride);
        if (waves == 0) { ctx->err = "the Counter table of one block (" + std::to_string(tk.stride) + " B) does not fit the device budget"; return 0; }
        o_P = meta + up256(waves * tk.stride);
        if (o_P + 256 >= budget || !aoh_plan(L.data(), nb, budget - o_P - 256, ctx->aoh_batch_blocks, plan)) {
            ctx->err = "the bit string and probabilities of one block do not fit the device budget";
            return 0;
        }
        o_str = o_P + up256(2 * plan.max_p_steps);
        return o_str + plan.max_str_bytes;
    });
    if (rc) return rc;
    uint8_t *base = (uint8_t *)ctx->tables.p;
    HIPCHK(ctx, hipMemcpy(base, plan.str_off.data(), (size_t)nb * 8, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(base + (size_t)nb * 8, plan.p_off.data(), (size_t)nb * 8, hipMemcpyHostToDevice));
    a.code = P.d_codes; a.L = P.d_L;
    a.str_off = (const uint64_t *)base; a.p_off = a.str_off + nb;
    a.tables = base + meta; a.table_stride = tk.stride;
    a.ctx_mask = (uint32_t)((1ull << ctx_bits) - 1ull); a.use_hash = tk.use_hash; a.hash_slots = tk.use_hash ? (uint32_t)tk.slots : 0u;
    a.P = (uint16_t *)(base + o_P); a.str = base + o_str;
    hipEvent_t *evp = ctx->opt_timing ? ctx->jobs[0].ev : nullptr;
    for (const AohBatch &bt : plan.batches) {   // (the batches share the string area and P: stream order keeps them apart)
        a.first_block = bt.first; a.count = bt.count;
        if (evp) HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PREDICT], s));
        hipLaunchKernelGGL(k_aoh_pack, dim3(std::min<uint32_t>(bt.count, 256u * 32u)), dim3(64), 0, s, a);
        hipLaunchKernelGGL(k_aoh_predict, dim3((unsigned)std::min<uint64_t>(bt.count, waves)), dim3(64), 0, s, a);
        if (evp) { HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PREDICT + 1], s)); HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_CODER], s)); }
        hipLaunchKernelGGL(k_aoh_coder<STATS>, dim3((bt.count + 63u) / 64u), dim3(64), 0, s, a);
        HIPCHK(ctx, hipGetLastError());
        if (evp) {
            HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_CODER + 1], s));
            HIPCHK(ctx, hipStreamSynchronize(s));
            ctx->timing.predict_ms += elapsed_ev(evp, W3_EV_PREDICT); ctx->timing.coder_ms += elapsed_ev(evp, W3_EV_CODER);
        }
        // algorithmic bytes: pack reads the input and writes the string; predict reads it, reads and writes one Counter per step and
        // writes 2 bytes of P; the coder reads P and the string
        const uint64_t in_bytes = std::min<uint64_t>(a.n, (uint64_t)(bt.first + bt.count) * a.block_size) - (uint64_t)bt.first * a.block_size;
        ctx->timing.predict_bytes += in_bytes + 2 * bt.str_bytes + bt.p_steps * (2 + 8);
        ctx->timing.coder_bytes += 2 * bt.p_steps + bt.str_bytes;
        ctx->timing.n_coder_launches++;
    }
    return W3_OK;
}

// Code blocks [0, nb) of d_in into ctx->jobs[0].stripes (stride cap_out), lengths to d_lens; d_bits (or null) gets the ACStats bit counts.
// two: the form the call took (aoh_takes_twophase).
static int aoh_encode_stripes(w3_ctx *ctx, hipStream_t s, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t n, size_t block_size,
                              uint32_t nb, uint32_t *d_lens, uint32_t *d_bits, uint32_t &cap_out, bool &two) {
    AohPrep P;
    int rc = aoh_prepare(ctx, s, code, 1, 1, nb, d_in, n, block_size, P);
    if (rc) return rc;
    if (P.flags[0]) { ctx->err = "the input holds a byte whose code length is 0: the output could not be decoded"; return W3_E_INVALID; }
    two = aoh_takes_twophase(ctx, nb, ctx_bits, P.max_l[0]);
    const w3_timing tm0 = ctx->timing;   // (a retry at the worst-case bound starts the call's sums again)
    // a Counter-coded stream rarely exceeds the Huffman bits it codes; 16 output bits per coded bit is the hard bound (retry size)
    const uint64_t l_bytes = ((uint64_t)P.max_l[0] + 7) / 8;
    const uint64_t worst = (16 * l_bytes + 16 + 15) / 16 * 16;
    if (worst > 0xFFFFFFF0ull) { ctx->err = "block too large for the worst-case stripe"; return W3_E_UNSUPPORTED; }
    uint64_t cap = std::min<uint64_t>((2 * l_bytes + 64 + 15) / 16 * 16, worst);
    ENSURE(ctx, ctx->jobs[0].flag, 16);
    std::vector<AohCfg> cfg(1);
    std::vector<uint64_t> steps(1, P.max_l[0]);
    for (int attempt = 0; attempt < 2; attempt++) {
        ENSURE(ctx, ctx->jobs[0].stripes, (size_t)nb * cap);
        HIPCHK(ctx, hipMemsetAsync(ctx->jobs[0].flag.p, 0, 16, s));
        if (two) {
            ctx->timing = tm0;
            AohTwoArgs t;
            memset(&t, 0, sizeof t);
            t.in = d_in; t.n = n; t.block_size = (uint32_t)block_size;
            t.stripes = (uint8_t *)ctx->jobs[0].stripes.p; t.stripe_cap = (uint32_t)cap; t.out_len = d_lens; t.overflow = (uint32_t *)ctx->jobs[0].flag.p; t.out_bits = d_bits;
            if ((rc = aoh_twophase_run<false>(ctx, s, t, P, ctx_bits, nb))) return rc;
        } else {
            memset(&cfg[0], 0, sizeof cfg[0]);
            cfg[0].ctx_bits = ctx_bits; cfg[0].code_idx = 0;
            AohArgs a;
            memset(&a, 0, sizeof a);
            a.in = d_in; a.n = n; a.block_size = (uint32_t)block_size;
            a.stripes = (uint8_t *)ctx->jobs[0].stripes.p; a.stripe_cap = (uint32_t)cap; a.out_len = d_lens; a.overflow = (uint32_t *)ctx->jobs[0].flag.p; a.out_bits = d_bits;
            if ((rc = aoh_launch<AOH_ENCODE>(ctx, s, a, P, cfg, steps, nb))) return rc;
        }
        uint32_t fl = 0;
        HIPCHK(ctx, hipMemcpyAsync(&fl, ctx->jobs[0].flag.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (!fl) { cap_out = (uint32_t)cap; return W3_OK; }
        if (cap == worst) break;
        cap = worst;
    }
    ctx->err = "stripe overflow at the worst-case bound (internal error)";
    return W3_E_HIP;
}

// (two: predict_ms / coder_ms and the byte counts are aoh_twophase_run's sums; generic_ms stays 0)
static void aoh_timing(w3_ctx *ctx, bool packed, bool two) {
    ctx->timing.path = two ? W3_PATH_TWOPHASE : W3_PATH_GENERIC; ctx->timing.n_parts = 1;
    if (!ctx->opt_timing) return;
    ctx->timing.generic_ms = two ? 0.f : elapsed_ev(ctx->jobs[0].ev, W3_EV_PREDICT);
    ctx->timing.pack_ms = packed ? elapsed_ev(ctx->jobs[0].ev, W3_EV_PACK) : 0.f;
    ctx->timing.total_ms = elapsed_ev(ctx->jobs[0].ev, W3_EV_TOTAL);
}

extern "C" int w3_aoh_encode_blocks_device(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t n, size_t block_size,
                                           uint8_t *d_out, size_t out_cap, uint32_t *d_block_lens, uint64_t *d_total, void *stream) {
    int rc = aoh_check(ctx, code, 1, &ctx_bits, 1, n, block_size, true);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint32_t nb = (uint32_t)((n + block_size - 1) / block_size);
    memset(&ctx->timing, 0, sizeof ctx->timing);
    ENSURE(ctx, ctx->total, 8);
    uint64_t *total_p = d_total ? d_total : (uint64_t *)ctx->total.p;
    if (nb == 0) {
        HIPCHK(ctx, hipMemsetAsync(total_p, 0, 8, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        return W3_OK;
    }
    if (!d_in || !d_block_lens || !d_out) return W3_E_INVALID;
    hipEvent_t *evp = ctx->opt_timing ? ctx->jobs[0].ev : nullptr;
    if (evp) { HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_TOTAL], s)); HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PREDICT], s)); }
    uint32_t cap = 0;
    bool two = false;
    if ((rc = aoh_encode_stripes(ctx, s, code, ctx_bits, d_in, n, block_size, nb, d_block_lens, nullptr, cap, two))) return rc;
    if (evp) { HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PREDICT + 1], s)); HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PACK], s)); }
    Job &J = ctx->jobs[0];
    if ((rc = run_pack(ctx, J, s, (const uint8_t *)ctx->jobs[0].stripes.p, cap, d_block_lens, nb, d_out, out_cap, total_p))) return rc;
    if (evp) { HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PACK + 1], s)); HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_TOTAL + 1], s)); }
    uint64_t total = 0;
    HIPCHK(ctx, hipMemcpyAsync(&total, total_p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    aoh_timing(ctx, true, two);
    if (total > out_cap) { ctx->err = "out_cap too small"; return W3_E_NOSPACE; }
    return W3_OK;
}

extern "C" int w3_aoh_encode_blocks(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t n, size_t block_size,
                                    uint8_t *out, size_t out_cap, size_t *out_len, uint32_t *block_lens) {
    int rc = aoh_check(ctx, code, 1, &ctx_bits, 1, n, block_size, false);
    if (rc) return rc;
    if (out_len) *out_len = 0;
    const size_t nb = (n + block_size - 1) / block_size;
    if (nb == 0) return W3_OK;
    if (!in || !block_lens || !out_len) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    memset(&ctx->timing, 0, sizeof ctx->timing);
    const size_t run = host_run_blocks(ctx, block_size);   // any length: device calls of at most 2 GiB of input, one after the other
    Job &J = ctx->jobs[0];
    size_t off = 0;
    uint32_t parts = 0;
    bool two = false;
    for (size_t b0 = 0; b0 < nb; b0 += run, parts++) {
        const size_t b1 = std::min(nb, b0 + run), lo = b0 * block_size, hi = std::min(n, b1 * block_size);
        const uint32_t pnb = (uint32_t)(b1 - b0);
        ENSURE(ctx, ctx->io_in, hi - lo);
        ENSURE(ctx, ctx->lens, (size_t)pnb * 4);
        ENSURE(ctx, ctx->total, 8);
        HIPCHK(ctx, hipMemcpyAsync(ctx->io_in.p, in + lo, hi - lo, hipMemcpyHostToDevice, s));
        uint32_t cap = 0;
        if ((rc = aoh_encode_stripes(ctx, s, code, ctx_bits, (const uint8_t *)ctx->io_in.p, hi - lo, block_size, pnb, (uint32_t *)ctx->lens.p, nullptr, cap, two))) return rc;
        // the piece's size first (the packed buffer is sized from it), then the pack
        ENSURE(ctx, J.offs, (size_t)pnb * 8);
        hipLaunchKernelGGL(k_scan_lens, dim3(1), dim3(1024), 0, s, (const uint32_t *)ctx->lens.p, (uint64_t *)J.offs.p, (uint64_t *)ctx->total.p, pnb);
        uint64_t total = 0;
        HIPCHK(ctx, hipMemcpyAsync(&total, ctx->total.p, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(block_lens + b0, ctx->lens.p, (size_t)pnb * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (out && off + total <= out_cap) {   // (once the caller's buffer is full the later pieces are still coded: *out_len must hold the need)
            ENSURE(ctx, ctx->io_out, (size_t)total);
            if ((rc = run_pack(ctx, J, s, (const uint8_t *)ctx->jobs[0].stripes.p, cap, (const uint32_t *)ctx->lens.p, pnb, (uint8_t *)ctx->io_out.p, (size_t)total, (uint64_t *)ctx->total.p))) return rc;
            HIPCHK(ctx, hipMemcpyAsync(out + off, ctx->io_out.p, (size_t)total, hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
        }
        off += (size_t)total;
    }
    ctx->timing.path = two ? W3_PATH_TWOPHASE : W3_PATH_GENERIC; ctx->timing.n_parts = parts;
    *out_len = off;
    if (off > out_cap || !out) { ctx->err = "out_cap too small"; return W3_E_NOSPACE; }
    return W3_OK;
}

// k_aoh_decode_spec (w3_aoh_spec.h) over jobs [0, nl): a direct table of 4 << ctx_bits bytes per job, as many jobs per batch (a
// multiple of 4: a wavefront takes four) as the budget of ensure_sweep_tables holds, W3_OPT_AOH_BATCH_BLOCKS caps a batch (tests);
// the tables are zero-filled per batch on the stream.
static int aoh_spec_launch(w3_ctx *ctx, hipStream_t s, AohSpecArgs a, uint8_t ctx_bits, uint32_t nl) {
    const uint64_t stride = std::max<uint64_t>(4ull << ctx_bits, 16);
    uint32_t per = 0;
    const int rc = ensure_sweep_tables(ctx, [&](uint64_t budget) {
        if (!(per = (uint32_t)lanes_per_batch(budget, stride, nl, ctx->aoh_batch_blocks, 4))) ctx->err = "the Counter table of one job does not fit the device budget";
        return per * stride;
    });
    if (rc) return rc;
    a.tables = (uint8_t *)ctx->tables.p; a.stride = stride; a.ctx_mask = (uint32_t)((1ull << ctx_bits) - 1ull);
    for (uint32_t first = 0; first < nl; first += per) {
        const uint32_t cnt = std::min(per, nl - first);
        HIPCHK(ctx, hipMemsetAsync(ctx->tables.p, 0, (size_t)(cnt * stride), s));
        a.first = first; a.count = cnt;
        hipLaunchKernelGGL(k_aoh_decode_spec, dim3((cnt + 3u) / 4u), dim3(64), 0, s, a);
        HIPCHK(ctx, hipGetLastError());
    }
    return W3_OK;
}

// which decoder a ranges call takes: the sixteen-lane kernel where it covers, unless W3_OPT_VARIANT bit 1024 asks for the lane kernel
static bool aoh_ranges_take_spec(const w3_ctx *ctx, uint8_t ctx_bits) {
    return aoh_spec_covers(ctx_bits) && !(ctx->opt.variant & W3_VAR_DECODE_LANE);
}
// ... and the full decode: the lane kernel, as before the sixteen-lane kernel existed, unless bit 2048 asks for that one (an untimed
// form does not become a default: DESIGN.md 7)
static bool aoh_full_take_spec(const w3_ctx *ctx, uint8_t ctx_bits) {
    return (ctx->opt.variant & W3_VAR_AOH_DECODE_SPEC) && aoh_ranges_take_spec(ctx, ctx_bits);
}

// The decoders of the family on device-resident streams (d_lens[nb], validated by the caller): every block whole into d_out
// (d_jobs == nullptr), or the n_jobs decode jobs of a ranges call (w3_ranges.h; the longest decodes max_job_len bytes) into d_out =
// the staging buffer.  spec: k_aoh_decode_spec, else k_aoh<AOH_DECODE>.  Does not synchronise after the launches.
// Precondition: ctx->coffs holds the exclusive scan of d_lens[nb], enqueued on s (scan_lens / check_len_table).
static int aoh_decode_run(w3_ctx *ctx, hipStream_t s, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_cin, const uint32_t *d_lens, uint32_t nb,
                          size_t block_size, uint64_t orig_len, uint8_t *d_out, const DecodeJob *d_jobs, uint32_t n_jobs, uint32_t max_job_len, bool spec) {
    int rc;
    const unsigned max_len = w3aoh::max_len(code);
    AohPrep P;
    if ((rc = aoh_prepare(ctx, s, code, 1, 1, nb, nullptr, (size_t)orig_len, block_size, P))) return rc;
    const uint32_t nl = d_jobs ? n_jobs : nb;
    if (spec) {
        AohSpecArgs sa;
        memset(&sa, 0, sizeof sa);
        sa.code = P.d_codes; sa.jobs = d_jobs; sa.n = orig_len; sa.block_size = (uint32_t)block_size;
        sa.cin = d_cin; sa.coffs = (const uint64_t *)ctx->coffs.p; sa.clens = d_lens; sa.dout = d_out;
        return aoh_spec_launch(ctx, s, sa, ctx_bits, nl);
    }
    std::vector<AohCfg> cfg(1);
    memset(&cfg[0], 0, sizeof cfg[0]);
    cfg[0].ctx_bits = ctx_bits;
    // the decoder does not know a stream's bit count before it has decoded it: the map is sized for the most steps a lane can take
    std::vector<uint64_t> steps(1, (uint64_t)(d_jobs ? max_job_len : std::min<uint64_t>(block_size, orig_len)) * max_len);
    AohArgs a;
    memset(&a, 0, sizeof a);
    a.n = orig_len; a.block_size = (uint32_t)block_size;
    a.cin = d_cin; a.coffs = (const uint64_t *)ctx->coffs.p; a.clens = d_lens; a.dout = d_out; a.jobs = d_jobs;
    return aoh_launch<AOH_DECODE>(ctx, s, a, P, cfg, steps, nl, d_jobs ? ctx->aoh_batch_blocks : 0u);
}

extern "C" int w3_aoh_decode_blocks_device(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t in_len,
                                           const uint32_t *d_block_lens, size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *d_out, void *stream) {
    int rc = aoh_check(ctx, code, 1, &ctx_bits, 1, (size_t)orig_len, block_size, true);
    if (rc) return rc;
    const uint64_t nb = (orig_len + block_size - 1) / block_size;
    if (nb != nblocks) { ctx->err = "nblocks does not match orig_len/block_size"; return W3_E_INVALID; }
    if (nb == 0) return W3_OK;
    if (!d_in || !d_block_lens || !d_out) return W3_E_INVALID;
    if (w3aoh::max_len(code) == 0) { ctx->err = "a table without symbols decodes nothing"; return W3_E_INVALID; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = check_len_table(ctx, s, d_block_lens, (uint32_t)nb, in_len))) return rc;
    const bool spec = aoh_full_take_spec(ctx, ctx_bits);
    if ((rc = aoh_decode_run(ctx, s, code, ctx_bits, d_in, d_block_lens, (uint32_t)nb, block_size, orig_len, d_out, nullptr, 0, 0, spec))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->timing.path = spec ? W3_PATH_SPEC : W3_PATH_GENERIC;
    return W3_OK;
}

// Random access on the family's streams (w3hip.h): the plan, the workspace and the gather are those of w3_decode_ranges[_device]
// (ranges_host / ranges_device), the decoder is aoh_decode_run over the plan's jobs.
static int aoh_ranges_check(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, size_t block_size, uint64_t orig_len, bool one_device, size_t *out_len) {
    if (out_len) *out_len = 0;
    int rc = aoh_check(ctx, code, 1, &ctx_bits, 1, (size_t)orig_len, block_size, one_device);
    if (rc) return rc;
    if (w3aoh::max_len(code) == 0) { ctx->err = "a table without symbols decodes nothing"; return W3_E_INVALID; }
    return out_len ? W3_OK : W3_E_INVALID;
}

static int aoh_decode_ranges_device_any(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t in_len,
                                        const uint32_t *d_block_lens, size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges,
                                        size_t n_ranges, uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream, w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    int rc = aoh_ranges_check(ctx, code, ctx_bits, block_size, orig_len, true, out_len);
    if (rc) return rc;
    RangeDec rd;
    CrcReport rep;
    rd.aoh_code = code; rd.aoh_ctx_bits = ctx_bits; rd.chk = chk; rd.rep = &rep;
    if ((rc = ranges_device(ctx, rd, d_in, in_len, d_block_lens, nblocks, block_size, orig_len, ranges, n_ranges, d_out, out_cap, out_len, stream))) return rc;
    ctx->timing.path = aoh_ranges_take_spec(ctx, ctx_bits) ? W3_PATH_SPEC : W3_PATH_GENERIC;
    return chk ? rep.finish(ctx, chk) : W3_OK;
}
extern "C" int w3_aoh_decode_ranges_device(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t in_len,
                                           const uint32_t *d_block_lens, size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges,
                                           size_t n_ranges, uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream) {
    return aoh_decode_ranges_device_any(ctx, code, ctx_bits, d_in, in_len, d_block_lens, nblocks, block_size, orig_len, ranges, n_ranges, d_out, out_cap, out_len, stream, nullptr);
}
extern "C" int w3_aoh_decode_ranges_device_checked(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t in_len,
                                                   const uint32_t *d_block_lens, size_t nblocks, size_t block_size, uint64_t orig_len,
                                                   const w3_range *ranges, size_t n_ranges, uint8_t *d_out, size_t out_cap, size_t *out_len, void *stream,
                                                   w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    if (out_len) *out_len = 0;
    if (const int rc = check_arg(ctx, chk)) return rc;
    return aoh_decode_ranges_device_any(ctx, code, ctx_bits, d_in, in_len, d_block_lens, nblocks, block_size, orig_len, ranges, n_ranges, d_out, out_cap, out_len, stream, chk);
}

static int aoh_decode_ranges_any(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                                 size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges, uint8_t *out,
                                 size_t out_cap, size_t *out_len, w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    int rc = aoh_ranges_check(ctx, code, ctx_bits, block_size, orig_len, false, out_len);   // (any length, as w3_decode_ranges)
    if (rc) return rc;
    RangeDec rd;
    CrcReport rep;
    rd.aoh_code = code; rd.aoh_ctx_bits = ctx_bits; rd.chk = chk; rd.rep = &rep;
    if ((rc = ranges_host(ctx, rd, in, in_len, block_lens, nblocks, block_size, orig_len, ranges, n_ranges, out, out_cap, out_len))) return rc;
    ctx->timing.path = aoh_ranges_take_spec(ctx, ctx_bits) ? W3_PATH_SPEC : W3_PATH_GENERIC;
    return chk ? rep.finish(ctx, chk) : W3_OK;
}
extern "C" int w3_aoh_decode_ranges(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                                    size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges, size_t n_ranges, uint8_t *out,
                                    size_t out_cap, size_t *out_len) {
    return aoh_decode_ranges_any(ctx, code, ctx_bits, in, in_len, block_lens, nblocks, block_size, orig_len, ranges, n_ranges, out, out_cap, out_len, nullptr);
}
extern "C" int w3_aoh_decode_ranges_checked(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len,
                                            const uint32_t *block_lens, size_t nblocks, size_t block_size, uint64_t orig_len, const w3_range *ranges,
                                            size_t n_ranges, uint8_t *out, size_t out_cap, size_t *out_len, w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    if (out_len) *out_len = 0;
    if (const int rc = check_arg(ctx, chk)) return rc;
    return aoh_decode_ranges_any(ctx, code, ctx_bits, in, in_len, block_lens, nblocks, block_size, orig_len, ranges, n_ranges, out, out_cap, out_len, chk);
}

extern "C" int w3_aoh_decode_spec_covers(uint8_t ctx_bits) { return aoh_spec_covers(ctx_bits) ? 1 : 0; }

static int aoh_decode_blocks_host(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                                 size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *out, w3_check *chk) {
    int rc = aoh_check(ctx, code, 1, &ctx_bits, 1, (size_t)orig_len, block_size, false);
    if (rc) return rc;
    if ((uint64_t)nblocks != (orig_len + block_size - 1) / block_size) { ctx->err = "nblocks does not match orig_len/block_size"; return W3_E_INVALID; }
    if (nblocks == 0) return W3_OK;
    if (!in || !block_lens || !out) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return host_decode_runs(ctx, in, in_len, block_lens, nblocks, block_size, orig_len, out, [&](const uint8_t *d_in, size_t len, const uint32_t *d_lens, size_t nb, uint64_t olen, uint8_t *d_out) {
        return w3_aoh_decode_blocks_device(ctx, code, ctx_bits, d_in, len, d_lens, nb, block_size, olen, d_out, ctx->stream);
    }, chk);
}
extern "C" int w3_aoh_decode_blocks(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len, const uint32_t *block_lens,
                                    size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *out) {
    return aoh_decode_blocks_host(ctx, code, ctx_bits, in, in_len, block_lens, nblocks, block_size, orig_len, out, nullptr);
}
extern "C" int w3_aoh_decode_blocks_checked(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t in_len,
                                            const uint32_t *block_lens, size_t nblocks, size_t block_size, uint64_t orig_len, uint8_t *out, w3_check *chk) {
    if (!ctx) return W3_E_INVALID;
    if (const int rc = check_arg(ctx, chk)) return rc;
    return aoh_decode_blocks_host(ctx, code, ctx_bits, in, in_len, block_lens, nblocks, block_size, orig_len, out, chk);
}

// the counting sink for configurations (codes[code_idx[c]], ctx_bits[c]) on a device-resident input: d_bits[ncfg][nb] (device).
// two (or null: the sweep, which stays on k_aoh whatever W3_OPT_PATH says): the form a one-configuration call took.
static int aoh_stats_run(w3_ctx *ctx, hipStream_t s, const uint8_t *d_in, size_t n, size_t block_size, uint32_t nb, const w3_huff_code *codes, size_t n_codes,
                         const uint8_t *code_idx, const uint8_t *ctx_bits, size_t ncfg, uint32_t *d_bits, bool *two) {
    AohPrep P;
    int rc = aoh_prepare(ctx, s, codes, n_codes, ncfg, nb, d_in, n, block_size, P);
    if (rc) return rc;
    if (two && (*two = ncfg == 1 && aoh_takes_twophase(ctx, nb, ctx_bits[0], P.max_l[0]))) {
        AohTwoArgs t;
        memset(&t, 0, sizeof t);
        t.in = d_in; t.n = n; t.block_size = (uint32_t)block_size; t.out_bits = d_bits;
        return aoh_twophase_run<true>(ctx, s, t, P, ctx_bits[0], nb);
    }
    std::vector<AohCfg> cfg(ncfg);
    std::vector<uint64_t> steps(ncfg);
    for (size_t c = 0; c < ncfg; c++) {
        memset(&cfg[c], 0, sizeof cfg[c]);
        cfg[c].ctx_bits = ctx_bits[c]; cfg[c].code_idx = code_idx ? code_idx[c] : 0;
        steps[c] = P.max_l[cfg[c].code_idx];
    }
    AohArgs a;
    memset(&a, 0, sizeof a);
    a.in = d_in; a.n = n; a.block_size = (uint32_t)block_size; a.out_bits = d_bits;
    return aoh_launch<AOH_STATS>(ctx, s, a, P, cfg, steps, nb);
}

extern "C" int w3_aoh_encode_stats_device(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *d_in, size_t n, size_t block_size,
                                          uint32_t *d_block_bits, void *stream) {
    int rc = aoh_check(ctx, code, 1, &ctx_bits, 1, n, block_size, true);
    if (rc) return rc;
    const size_t nb = (n + block_size - 1) / block_size;
    if (nb == 0) return W3_OK;
    if (!d_in || !d_block_bits) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    memset(&ctx->timing, 0, sizeof ctx->timing);
    hipEvent_t *evp = ctx->opt_timing ? ctx->jobs[0].ev : nullptr;
    if (evp) { HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_TOTAL], s)); HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PREDICT], s)); }
    bool two = false;
    if ((rc = aoh_stats_run(ctx, s, d_in, n, block_size, (uint32_t)nb, code, 1, nullptr, &ctx_bits, 1, d_block_bits, &two))) return rc;
    if (evp) { HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_PREDICT + 1], s)); HIPCHK(ctx, hipEventRecord(evp[2 * W3_EV_TOTAL + 1], s)); }
    HIPCHK(ctx, hipStreamSynchronize(s));
    aoh_timing(ctx, false, two);
    return W3_OK;
}

extern "C" int w3_aoh_encode_stats(w3_ctx *ctx, const w3_huff_code *code, uint8_t ctx_bits, const uint8_t *in, size_t n, size_t block_size,
                                   uint32_t *block_bits) {
    int rc = aoh_check(ctx, code, 1, &ctx_bits, 1, n, block_size, false);
    if (rc) return rc;
    const size_t nb = (n + block_size - 1) / block_size;
    if (nb == 0) return W3_OK;
    if (!in || !block_bits) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t run = host_run_blocks(ctx, block_size);
    for (size_t b0 = 0; b0 < nb; b0 += run) {
        const size_t b1 = std::min(nb, b0 + run), lo = b0 * block_size, hi = std::min(n, b1 * block_size);
        ENSURE(ctx, ctx->io_in, hi - lo);
        ENSURE(ctx, ctx->jobs[0].bits, (b1 - b0) * 4);
        HIPCHK(ctx, hipMemcpy(ctx->io_in.p, in + lo, hi - lo, hipMemcpyHostToDevice));
        if ((rc = w3_aoh_encode_stats_device(ctx, code, ctx_bits, (const uint8_t *)ctx->io_in.p, hi - lo, block_size, (uint32_t *)ctx->jobs[0].bits.p, ctx->stream))) return rc;
        HIPCHK(ctx, hipMemcpy(block_bits + b0, ctx->jobs[0].bits.p, (b1 - b0) * 4, hipMemcpyDeviceToHost));
    }
    return W3_OK;
}

// the driver's main (:13-44) as one call: every (huffman table, ctx_bits) x block through the counting sink
extern "C" int w3_sweep_ac_over_huffman_device(w3_ctx *ctx, const uint8_t *d_in, size_t n, size_t block_size, const w3_huff_code *codes, size_t n_codes,
                                               const uint8_t *code_idx, const uint8_t *ctx_bits, size_t ncfg, uint32_t *block_bits) {
    if (!ctx) return W3_E_INVALID;
    if (n_codes == 0 || n_codes > 64 || ncfg > 4096 || (ncfg && !code_idx)) { ctx->err = "1..64 code tables, at most 4096 configurations"; return W3_E_INVALID; }
    int rc = aoh_check(ctx, codes, n_codes, ctx_bits, ncfg, n, block_size, true);
    if (rc) return rc;
    for (size_t c = 0; c < ncfg; c++)
        if (code_idx[c] >= n_codes) { ctx->err = "code_idx out of range"; return W3_E_INVALID; }
    const uint32_t nb = (uint32_t)((n + block_size - 1) / block_size);
    if (nb == 0 || ncfg == 0) return W3_OK;
    if (!d_in || !block_bits) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    ENSURE(ctx, ctx->sweep, ncfg * (size_t)nb * 4);
    if ((rc = aoh_stats_run(ctx, s, d_in, n, block_size, nb, codes, n_codes, code_idx, ctx_bits, ncfg, (uint32_t *)ctx->sweep.p, nullptr))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(block_bits, ctx->sweep.p, ncfg * (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return W3_OK;
}

extern "C" int w3_sweep_ac_over_huffman(w3_ctx *ctx, const uint8_t *in, size_t n, size_t block_size, const w3_huff_code *codes, size_t n_codes,
                                        const uint8_t *code_idx, const uint8_t *ctx_bits, size_t ncfg, uint32_t *block_bits) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;
    if (n == 0 || ncfg == 0) return W3_OK;
    if (!in) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->io_in, n);
    HIPCHK(ctx, hipMemcpy(ctx->io_in.p, in, n, hipMemcpyHostToDevice));
    return w3_sweep_ac_over_huffman_device(ctx, (const uint8_t *)ctx->io_in.p, n, block_size, codes, n_codes, code_idx, ctx_bits, ncfg, block_bits);
}

// ---------------------------------------------------------------------------
// Context statistics export (README.md:9 "output stats from contexts for use by external neural nets"): the Counter table of a
// Counter-table model after it has seen the whole input as ONE stream — what `stats` of models/ordern.rs:5 holds when the
// reference's compress() returns.  One serial chain (one lane, as w3_compress_stream).
// ---------------------------------------------------------------------------
extern "C" int w3_export_counters(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, uint32_t *counters) {
    if (!ctx || !counters) return W3_E_INVALID;
    ParsedSpec ps;
    int rc = jobs_idle(ctx);
    if (rc) return rc;
    if ((rc = parse_spec(spec, ps))) return rc;
    if (ps.n_leaves != 1 || ps.n_apm || ps.has_slot || ps.leaf[0].frozen) { ctx->err = "w3_export_counters takes ONE adaptive Counter-table leaf"; return W3_E_UNSUPPORTED; }
    const w3_node &nd = ps.leaf[0];
    if (ps.has_match) { ctx->err = "w3_export_counters: the match-model leaf (W3_HIST_MATCH) is not exported"; return W3_E_UNSUPPORTED; }
    if (nd.bits > 28) { ctx->err = "tables above 2^28 counters are not exported"; return W3_E_UNSUPPORTED; }
    if (n > (1u << 28)) { ctx->err = "single-stream export limited to 2^28 bytes"; return W3_E_UNSUPPORTED; }
    const size_t entries = (size_t)1 << nd.bits;
    if (n == 0) { memset(counters, 0, entries * 4); return W3_OK; }
    if (!in) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if ((rc = stage_huff(ctx, s, ps))) return rc;
    CmArgs ca;
    memset(&ca, 0, sizeof ca);
    GenericArgs &ga = ca.g;
    (void)layout_generic(ps, n, ga);
    ga.leaf[0].use_hash = 0; ga.leaf[0].tbl_off = 0;            // direct-indexed, like the reference's Vec<Counter>
    if ((rc = prepare_achash_luts(ctx, s, ga))) return rc;
    const uint32_t cap = default_stripe_cap(n);
    ENSURE(ctx, ctx->tables, entries * 4);
    ENSURE(ctx, ctx->io_in, n);
    ENSURE(ctx, ctx->jobs[0].stripes, cap);
    ENSURE(ctx, ctx->lens, 4);
    ENSURE(ctx, ctx->jobs[0].flag, 16);
    HIPCHK(ctx, hipMemcpyAsync(ctx->io_in.p, in, n, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemsetAsync(ctx->tables.p, 0, entries * 4, s));
    ga.n = n; ga.block_size = (uint32_t)n; ga.first_block = 0; ga.n_lanes = 1;
    ga.huff = lane_huff(ctx, ps); ga.n_huff = (int)ps.n_huff;
    ga.tables = (uint8_t *)ctx->tables.p; ga.lane_stride = entries * 4;
    ga.in = (const uint8_t *)ctx->io_in.p; ga.stripes = (uint8_t *)ctx->jobs[0].stripes.p; ga.stripe_cap = cap;
    ga.out_len = (uint32_t *)ctx->lens.p; ga.overflow = (uint32_t *)ctx->jobs[0].flag.p; ga.out_bits = nullptr;
    lane_launch<false>(ca, 1, s, false);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(counters, ctx->tables.p, entries * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return W3_OK;
}

// ---------------------------------------------------------------------------
// The same on the device for whole inputs of any size (w3_export.h, w3_export_entropy.h): ONE adaptive leaf; count, apply and replay per
// epoch, for ACHistory and HuffHistory behind a key stage per epoch.  w3_export_counters_device / _staged admit OrderN leaves without
// entropy history only, w3_export_entropy_device / _staged every history; behind the argument check they are one path.
// ---------------------------------------------------------------------------
static int export_args(w3_ctx *ctx, const w3_model_spec *spec, const void *in, size_t n, const void *out, bool one_device, bool admits_entropy, ParsedSpec &ps,
                       ExpModel &m) {
    int rc = check_args(ctx, n, W3_PREP_NOMINAL_BLOCK, one_device);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;   // (the workspace is the context's)
    if ((rc = parse_spec(spec, ps))) return rc;
    if (ps.n_leaves != 1 || ps.n_apm || ps.has_slot || ps.leaf[0].kind != W3_NODE_ORDERN || ps.leaf[0].frozen ||
        (admits_entropy ? ps.leaf[0].history > W3_HIST_HUFF : ps.leaf[0].history != W3_HIST_NONE)) {
        ctx->err = admits_entropy
                       ? "w3_export_entropy_device / _staged take ONE adaptive OrderN or OrderNEntropy leaf (RawHistory, ACHistory, HuffHistory)"
                       : "the parallel export takes ONE adaptive OrderN leaf without entropy history: w3_export_counters (one lane) or w3_export_entropy_device / _staged (in parallel) are the routes for leaves with an entropy history";
        return W3_E_UNSUPPORTED;
    }
    if (ps.leaf[0].bits > W3_EXP_MAX_BITS) { ctx->err = "tables above 2^28 counters are not exported"; return W3_E_UNSUPPORTED; }
    if (!out || (!in && n)) return W3_E_INVALID;
    m.bits = ps.leaf[0].bits; m.align = ps.leaf[0].align;
    if (admits_entropy) ctx->exp_prof = w3_export_entropy_profile();
    else ctx->exp_prof.base = w3_export_profile();   // (a counters call leaves what only an entropy call reports)
    return W3_OK;
}

// the workspace for a stream of `upto` bytes: D (zero), the replay list, the stats words
static int export_ensure(w3_ctx *ctx, hipStream_t s, const ExpModel &m, uint64_t upto) {
    const size_t need = (size_t)8 << m.bits;
    const void *had = ctx->exp_d.p;
    ENSURE(ctx, ctx->exp_d, need);
    if (ctx->exp_d.p != had) ctx->exp_d_zero = 0;
    if (ctx->exp_d_zero < need) {
        HIPCHK(ctx, hipMemsetAsync(ctx->exp_d.p, 0, need, s));
        ctx->exp_d_zero = need;
    }
    ENSURE(ctx, ctx->exp_list, (size_t)exp_list_cap(m.bits, upto) * 4);
    ENSURE(ctx, ctx->exp_stats, W3_EXP_ST_WORDS * 4);
    return W3_OK;
}

// What a leaf with an entropy history adds (w3_export_entropy.h): the key stage's arguments
struct ExpKeyed {
    int history;                // W3_HIST_AC or W3_HIST_HUFF
    uint32_t max_bits; uint16_t table[8]; const uint4 *lut;   // ACHistory
    const w3_huff_table *tb;                                  // HuffHistory (on the device)
    const w3_huff_table *host_tb;                             // ... and the caller's (the staged form's seed chain)
};
static uint64_t export_epoch_bytes(const w3_ctx *ctx, bool keyed) {
    if (!keyed) return ctx->export_epoch ? ctx->export_epoch : W3_EXP_EPOCH_DEFAULT;
    return ctx->export_epoch ? std::min<uint64_t>(ctx->export_epoch, W3_EXPK_EPOCH_MAX) : W3_EXPK_EPOCH_DEFAULT;
}

// the key stage's workspace and tables for pieces of at most `piece` bytes; false in `keyed`: the leaf needs none (OrderN, RawHistory)
static int export_keyed_prepare(w3_ctx *ctx, hipStream_t s, const ParsedSpec &ps, size_t piece, ExpKeyed &kd, bool &keyed) {
    const w3_node &nd = ps.leaf[0];
    keyed = nd.history == W3_HIST_AC || nd.history == W3_HIST_HUFF;
    if (!keyed) return W3_OK;
    memset(&kd, 0, sizeof kd);
    kd.history = nd.history;
    int rc;
    if (nd.history == W3_HIST_HUFF) {
        if ((rc = stage_huff(ctx, s, ps))) return rc;
        kd.tb = lane_huff(ctx, ps) + nd.reserved;
        kd.host_tb = ps.huff + nd.reserved;
        ENSURE(ctx, ctx->exp_hs, W3_EXPK_HS_WORDS * 4);
    } else {
        GenericArgs ga;
        memset(&ga, 0, sizeof ga);
        (void)layout_generic(ps, W3_PREP_NOMINAL_BLOCK, ga);
        if ((rc = prepare_achash_luts(ctx, s, ga))) return rc;
        kd.lut = ga.leaf[0].lut; kd.max_bits = nd.max_bits;
        memcpy(kd.table, nd.table, sizeof kd.table);
    }
    ENSURE(ctx, ctx->exp_k, (size_t)std::min<uint64_t>(export_epoch_bytes(ctx, true), (piece + 1023) / 1024 * 1024) * 32);
    return W3_OK;
}

// the key stage of the epoch [e0, e0 + len): K = ctx | bit << 31 per step
static void export_launch_keys(w3_ctx *ctx, hipStream_t s, const ExpKeyed &kd, const ExpPiece &pc, uint64_t e0, uint64_t len, const ExpModel &m) {
    uint32_t *K = (uint32_t *)ctx->exp_k.p;
    if (kd.history == W3_HIST_AC) {
        ExpAcArgs a;
        memset(&a, 0, sizeof a);
        a.pc = pc; a.e0 = e0; a.len = len; a.m = m; a.max_bits = kd.max_bits; a.lut = kd.lut; a.K = K;
        memcpy(a.table, kd.table, sizeof a.table);
        hipLaunchKernelGGL(k_expk_ackeys, dim3((unsigned)std::min<uint64_t>((len * 8 + 255) / 256, 1u << 20)), dim3(256), 0, s, a);
    } else {
        ExpHuffArgs a;
        memset(&a, 0, sizeof a);
        a.pc = pc; a.e0 = e0; a.len = len; a.m = m; a.tb = kd.tb; a.K = K; a.hs = (uint32_t *)ctx->exp_hs.p;
        hipLaunchKernelGGL(k_expk_huffkeys, dim3((unsigned)std::min<uint64_t>((len + 255) / 256, 1u << 16)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_expk_huff_fix, dim3(1), dim3(64), 0, s, a);
    }
}

// count and replay over a source; rows_per_wg: the rows a workgroup of the count has in flight
template <class Src>
static void export_launch_count(w3_ctx *ctx, hipStream_t s, const Src &src, uint64_t rows_per_wg, const ExpModel &m) {
    const uint64_t wgs = (exp_rows(src) + rows_per_wg - 1) / rows_per_wg;
    exp_u64 *D = (exp_u64 *)ctx->exp_d.p;
    uint32_t *stats = (uint32_t *)ctx->exp_stats.p;
    if (m.bits <= W3_EXP_LDS_BITS)
        hipLaunchKernelGGL((k_exp_count_lds<Src, W3_EXP_LDS_REP>), dim3((uint32_t)std::min<uint64_t>(wgs, W3_EXP_LDS_MAX_WG)), dim3(256),
                           (size_t)(8u << m.bits) * W3_EXP_LDS_REP, s, src, m.bits, D, stats);
    else
        hipLaunchKernelGGL(k_exp_count<Src>, dim3((uint32_t)std::min<uint64_t>(wgs, W3_EXP_GLOBAL_MAX_WG)), dim3(256), 0, s, src, D, stats);
}
template <class Src>
static void export_launch_replay(w3_ctx *ctx, hipStream_t s, const Src &src, uint32_t *S, uint32_t cap) {
    hipLaunchKernelGGL(k_exp_replay<Src>, dim3(std::min<uint32_t>(cap, W3_EXP_REPLAY_MAX_WG)), dim3(64), 0, s, src, S, (const uint32_t *)ctx->exp_list.p, cap,
                       (uint32_t *)ctx->exp_stats.p);
}

// One piece that lies on the device through its epochs, S = the table before it and behind it; synchronises s.  The list's bound is that
// of the stream's bytes through this piece's end.  Adds to ctx->exp_prof.  kd: the keyed form (a key stage per epoch, count and replay
// over the keys).
static int export_piece(w3_ctx *ctx, hipStream_t s, const ExpPiece &pc, const ExpModel &m, uint32_t *S, const ExpKeyed *kd) {
    const uint64_t E = export_epoch_bytes(ctx, kd != nullptr), nctx = 1ull << m.bits;
    const size_t nst = kd ? 4 : 3;   // kernels (timed stages) per epoch
    const bool huff = kd && kd->history == W3_HIST_HUFF;
    const uint64_t epochs = (pc.n + E - 1) / E;
    const uint32_t cap = (uint32_t)exp_list_cap(m.bits, pc.abs0 + pc.n);
    uint32_t *stats = (uint32_t *)ctx->exp_stats.p;
    const size_t zero_had = ctx->exp_d_zero;
    ctx->exp_d_zero = 0;   // (until the piece is through: a failed call leaves D in an unknown state)
    std::vector<hipEvent_t> ev;
    struct Events {   // destroyed on every way out
        std::vector<hipEvent_t> &v;
        ~Events() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
    } events{ev};
    const bool per_kernel = ctx->opt_timing && epochs <= 4096;
    if (ctx->opt_timing) {
        ev.resize(per_kernel ? nst * (size_t)epochs + 1 : 2, nullptr);
        for (auto &e : ev) HIPCHK(ctx, hipEventCreate(&e));
        HIPCHK(ctx, hipEventRecord(ev[0], s));
    }
    HIPCHK(ctx, hipMemsetAsync(stats, 0, W3_EXP_ST_WORDS * 4, s));
    if (huff) HIPCHK(ctx, hipMemsetAsync(ctx->exp_hs.p, 0, W3_EXPK_HS_WORDS * 4, s));
    const uint32_t apply_wg = (uint32_t)std::min<uint64_t>((nctx + 255) / 256, 8192);
    for (uint64_t k = 0; k < epochs; k++) {
        const uint64_t e0 = k * E, len = std::min<uint64_t>(E, pc.n - e0);
        const ExpRawSrc raw = {pc, e0, len, m};
        const ExpKeySrc keys = {(const uint32_t *)ctx->exp_k.p, len * 8};
        size_t at = nst * k;   // the epoch's first event
        auto stage_done = [&]() -> int {
            HIPCHK(ctx, hipGetLastError());
            if (per_kernel) HIPCHK(ctx, hipEventRecord(ev[++at], s));
            return W3_OK;
        };
        int rc;
        if (kd) {
            export_launch_keys(ctx, s, *kd, pc, e0, len, m);
            if ((rc = stage_done())) return rc;
            export_launch_count(ctx, s, keys, 4u * W3_EXPK_COUNT_ROWS, m);
        } else {
            export_launch_count(ctx, s, raw, 4u, m);
        }
        if ((rc = stage_done())) return rc;
        hipLaunchKernelGGL(k_ctx_apply, dim3(apply_wg), dim3(256), 0, s, (exp_u64 *)ctx->exp_d.p, S, nctx, (uint32_t *)ctx->exp_list.p, cap, stats);
        if ((rc = stage_done())) return rc;
        if (kd) export_launch_replay(ctx, s, keys, S, cap);
        else export_launch_replay(ctx, s, raw, S, cap);
        if ((rc = stage_done())) return rc;
    }
    if (ctx->opt_timing && !per_kernel) HIPCHK(ctx, hipEventRecord(ev[1], s));
    uint32_t st[W3_EXP_ST_WORDS] = {0};
    uint32_t hst[W3_EXPK_HS_WORDS] = {0};
    HIPCHK(ctx, hipMemcpyAsync(st, stats, sizeof st, hipMemcpyDeviceToHost, s));
    if (huff) HIPCHK(ctx, hipMemcpyAsync(hst, ctx->exp_hs.p, sizeof hst, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->exp_prof.huff_fixed_epochs += hst[W3_EXPK_HS_FIXED];
    if (st[W3_EXP_ST_OVERFLOW]) { ctx->err = "the export's replay list exceeded its bound"; return W3_E_HIP; }
    ctx->exp_d_zero = zero_had;   // (k_ctx_apply zeroed what the count added)
    w3_export_profile &pr = ctx->exp_prof.base;
    pr.epochs += epochs; pr.replays += st[W3_EXP_ST_REPLAYS]; pr.halvings += st[W3_EXP_ST_HALVINGS];
    if (ctx->opt_timing) {
        float ms = 0.f;
        if (per_kernel)
            for (uint64_t k = 0; k < epochs; k++) {
                float *into[4] = {&ctx->exp_prof.key_ms, &pr.count_ms, &pr.apply_ms, &pr.replay_ms};
                for (size_t j = 0; j < nst; j++) { HIPCHK(ctx, hipEventElapsedTime(&ms, ev[nst * k + j], ev[nst * k + j + 1])); *into[4 - nst + j] += ms; }
            }
        HIPCHK(ctx, hipEventElapsedTime(&ms, ev.front(), ev.back()));
        pr.total_ms += ms;
    }
    return W3_OK;
}

static int export_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, uint32_t *d_counters, void *stream, bool admits_entropy) {
    ExpModel m;
    ParsedSpec ps;
    int rc = export_args(ctx, spec, d_in, n, d_counters, true, admits_entropy, ps, m);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(d_counters, 0, (size_t)4 << m.bits, s));
    if (n == 0) { HIPCHK(ctx, hipStreamSynchronize(s)); return W3_OK; }
    if ((rc = export_ensure(ctx, s, m, n))) return rc;
    ExpKeyed kd;
    bool keyed = false;
    if ((rc = export_keyed_prepare(ctx, s, ps, n, kd, keyed))) return rc;
    const ExpPiece pc = {d_in, n, 0, 0, 0};
    return export_piece(ctx, s, pc, m, d_counters, keyed ? &kd : nullptr);
}

static int export_staged(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, uint32_t *counters, bool admits_entropy) {
    ExpModel m;
    ParsedSpec ps;
    int rc = export_args(ctx, spec, in, n, counters, false, admits_entropy, ps, m);
    if (rc) return rc;
    const size_t bytes = (size_t)4 << m.bits;
    if (n == 0) { memset(counters, 0, bytes); return W3_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t piece = host_run_blocks(ctx, W3_PREP_NOMINAL_BLOCK) * (size_t)W3_PREP_NOMINAL_BLOCK;
    if ((rc = export_ensure(ctx, s, m, n))) return rc;
    ExpKeyed kd;
    bool keyed = false;
    if ((rc = export_keyed_prepare(ctx, s, ps, std::min(n, piece), kd, keyed))) return rc;
    const w3_huff_table *tb = keyed ? kd.host_tb : nullptr;   // (HuffHistory only)
    ENSURE(ctx, ctx->exp_s, bytes);
    ENSURE(ctx, ctx->io_in, std::min(n, piece));
    HIPCHK(ctx, hipMemsetAsync(ctx->exp_s.p, 0, bytes, s));
    uint32_t seed = 0;   // HuffHistory's compressed_bits at the piece's first byte
    for (size_t o0 = 0; o0 < n; o0 += piece) {
        const size_t len = std::min(piece, n - o0);
        uint64_t carry = 0;   // the eight stream bytes before the piece
        for (size_t k = o0 < 8 ? 0 : o0 - 8; k < o0; k++) carry = (carry << 8) | in[k];
        if (tb && o0) seed = expk_huff_piece_seed(in, o0, o0 - piece, seed, tb->code, tb->len);
        HIPCHK(ctx, hipMemcpyAsync(ctx->io_in.p, in + o0, len, hipMemcpyHostToDevice, s));
        const ExpPiece pc = {(const uint8_t *)ctx->io_in.p, len, o0, carry, seed};
        if ((rc = export_piece(ctx, s, pc, m, (uint32_t *)ctx->exp_s.p, keyed ? &kd : nullptr))) return rc;   // (synchronises: the next piece overwrites io_in)
    }
    HIPCHK(ctx, hipMemcpy(counters, ctx->exp_s.p, bytes, hipMemcpyDeviceToHost));
    return W3_OK;
}

extern "C" int w3_export_counters_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, uint32_t *d_counters, void *stream) {
    return export_device(ctx, spec, d_in, n, d_counters, stream, false);
}
extern "C" int w3_export_counters_staged(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, uint32_t *counters) {
    return export_staged(ctx, spec, in, n, counters, false);
}
extern "C" int w3_export_entropy_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, uint32_t *d_counters, void *stream) {
    return export_device(ctx, spec, d_in, n, d_counters, stream, true);
}
extern "C" int w3_export_entropy_staged(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, uint32_t *counters) {
    return export_staged(ctx, spec, in, n, counters, true);
}

extern "C" int w3_export_get_profile(const w3_ctx *ctx, w3_export_profile *out) {
    if (!ctx || !out) return W3_E_INVALID;
    *out = ctx->exp_prof.base;
    return W3_OK;
}
extern "C" int w3_export_entropy_get_profile(const w3_ctx *ctx, w3_export_entropy_profile *out) {
    if (!ctx || !out) return W3_E_INVALID;
    *out = ctx->exp_prof;
    return W3_OK;
}

// ---------------------------------------------------------------------------
// HuffHistory::new (history/huff_history.rs:17-55): constructor-time table prep on the host (w3_huff.h)
// ---------------------------------------------------------------------------
extern "C" int w3_huff_tables(const uint8_t *buf, size_t n, uint8_t huff_size, uint8_t rem_huff_size, w3_huff_table *out) {
    if ((!buf && n) || !out) return W3_E_INVALID;
    if (huff_size > 16 || rem_huff_size > 16) return W3_E_INVALID;   // codes are u16 (package_merge.rs:87: Vec<(u16, u8)>)
    uint64_t c64[256] = {0};
    for (size_t i = 0; i < n; i++) c64[buf[i]]++;
    return w3_huff_tables_from_counts(c64, huff_size, rem_huff_size, out);
}

// ... from the histogram alone: the one builder of the two tables
extern "C" int w3_huff_tables_from_counts(const uint64_t c64[256], uint8_t huff_size, uint8_t rem_huff_size, w3_huff_table *out) {
    if (!c64 || !out) return W3_E_INVALID;
    if (huff_size > 16 || rem_huff_size > 16) return W3_E_INVALID;
    uint32_t counts[256];
    if (const int rc = counts_to_u32(c64, counts)) return rc;
    return w3huff::build(counts, huff_size, rem_huff_size, out) ? W3_OK : W3_E_INVALID;
}

// ---------------------------------------------------------------------------
// Model::predict for every step (two-phase predict kernels only)
// ---------------------------------------------------------------------------
extern "C" int w3_predict_blocks(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, size_t block_size, uint16_t *p_out) {
    int rc = check_args(ctx, n, block_size);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;   // (the predict phase runs on job 0's workspace)
    ParsedSpec ps;
    if ((rc = parse_spec(spec, ps))) return rc;
    if (n == 0) return W3_OK;
    if (!in || !p_out) return W3_E_INVALID;
    if (!twophase_supported(ps, block_size, n)) { ctx->err = "spec not covered by the two-phase predict kernels"; return W3_E_UNSUPPORTED; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (ps.is_cm() && (rc = stage_cm_luts(ctx, s))) return rc;
    const uint32_t nb = (uint32_t)((n + block_size - 1) / block_size);
    if ((rc = stage_huff(ctx, s, ps))) return rc;
    hand_options(ctx, ctx->jobs[0], true);
    ENSURE(ctx, ctx->io_in, n);
    HIPCHK(ctx, hipMemcpyAsync(ctx->io_in.p, in, n, hipMemcpyHostToDevice, s));
    const uint16_t *d_p = nullptr;
    if ((rc = attach_aux_streams(ctx, ctx->jobs[0]))) return rc;
    rc = twophase_predict(ctx->jobs[0].tp, s, ps, (const uint8_t *)ctx->io_in.p, n, block_size, nb, ps.n_apm == 0 && !ps.has_mix, &d_p, nullptr, &ctx->timing, ctx->err);
    if (rc) return rc;
    if ((rc = twophase_lmix(ctx->jobs[0].tp, s, ps, (const uint8_t *)ctx->io_in.p, n, block_size, nb, nullptr, &ctx->timing, ctx->err))) return rc;
    if ((rc = twophase_apm(ctx->jobs[0].tp, s, ps, (const uint8_t *)ctx->io_in.p, n, block_size, nb, nullptr, &ctx->timing, ctx->err))) return rc;
    d_p = (const uint16_t *)ctx->jobs[0].tp.P;
    HIPCHK(ctx, hipStreamSynchronize(s));
    HIPCHK(ctx, hipMemcpy(p_out, d_p, n * 16, hipMemcpyDeviceToHost));
    return W3_OK;
}

// ---------------------------------------------------------------------------
// per-step statistics export (include/w3hip.h: w3_export_steps_device; csrc/w3_steps.h)
// ---------------------------------------------------------------------------
extern "C" int w3_steps_layout_of(const w3_model_spec *spec, uint32_t format, uint32_t flags, w3_steps_layout *out) {
    if (!out) return W3_E_INVALID;
    ParsedSpec ps;
    if (const int rc = parse_spec(spec, ps)) return rc;
    if (ps.has_mix) return W3_E_UNSUPPORTED;   // (the rows' mix column is OpinionMixer2's: steps_args)
    StepsLayout l;
    if (!steps_layout((uint32_t)ps.n_leaves, (uint32_t)ps.n_apm, format, flags, l)) return W3_E_INVALID;
    out->n_cols = l.n_cols; out->n_leaves = l.n_leaves; out->col_mix = l.col_mix; out->col_apm0 = l.col_apm0; out->n_apm = l.n_apm;
    out->col_final = l.col_final; out->col_bit = l.col_bit; out->elem_bytes = l.elem_bytes;
    return W3_OK;
}

template <bool STAGED>
static void steps_launch(uint32_t C, dim3 grid, uint32_t lds, hipStream_t s, const StepsArgs &a) {
    switch (C) {   // (the bench model with the bit column has 6 columns, init_model() 3)
    case 2: hipLaunchKernelGGL((k_steps_rows<2, STAGED>), grid, dim3(64), lds, s, a); break;
    case 3: hipLaunchKernelGGL((k_steps_rows<3, STAGED>), grid, dim3(64), lds, s, a); break;
    case 4: hipLaunchKernelGGL((k_steps_rows<4, STAGED>), grid, dim3(64), lds, s, a); break;
    case 5: hipLaunchKernelGGL((k_steps_rows<5, STAGED>), grid, dim3(64), lds, s, a); break;
    case 6: hipLaunchKernelGGL((k_steps_rows<6, STAGED>), grid, dim3(64), lds, s, a); break;
    case 7: hipLaunchKernelGGL((k_steps_rows<7, STAGED>), grid, dim3(64), lds, s, a); break;
    case 8: hipLaunchKernelGGL((k_steps_rows<8, STAGED>), grid, dim3(64), lds, s, a); break;
    default: hipLaunchKernelGGL((k_steps_rows<0, STAGED>), grid, dim3(64), lds, s, a); break;
    }
}

// The rows of n input bytes (whole blocks but for the last) at d_in into d_rows, on job 0's workspace: the predict phase, the sampled
// verification of its LDS-add rounds exactly as an encode runs it, the APM stages ONE AT A TIME with a copy of ws.P after each, the row
// kernel.  Synchronous.  prof: the call's times and counts are ADDED (the staged form sums its pieces).
static int steps_run(w3_ctx *ctx, hipStream_t s, const ParsedSpec &ps, const StepsLayout &lay, uint32_t format, const uint8_t *d_in, size_t n,
                     size_t block_size, void *d_rows, w3_steps_profile &prof) {
    Job &J = ctx->jobs[0];
    TwoPhaseWs &ws = J.tp;
    const uint32_t nb = (uint32_t)((n + block_size - 1) / block_size);
    int rc;
    if ((rc = job_prepare(ctx, J, ps, s, true, false, n, block_size, nb))) return rc;
    if (!ctx->stretch && (rc = stage_cm_luts(ctx, s))) return rc;   // (the formats' table: job_prepare stages it only for models that use it)
    ws.stretch = ctx->stretch; ws.squash = ctx->squash;
    int n_live = 0;
    for (int l = 0; l < ps.n_leaves; l++) n_live += leaf_class(ps.leaf[l]) != LEAF_FROZEN;
    // ws.P is rewritten by every stage, and by the first one IN PLACE where a single live leaf wrote its stream there: copies
    const bool leaf_in_P = n_live == 1 && ps.n_apm > 0;
    const size_t n_copies = (leaf_in_P ? 1 : 0) + (ps.n_apm > 1 ? (size_t)ps.n_apm - 1 : 0);
    ENSURE(ctx, ctx->steps_copies, n_copies * n * 16);
    hipEvent_t *ev = ctx->opt_timing ? J.ev : nullptr;
    uint32_t lds_faults = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        HIPCHK(ctx, hipMemsetAsync(J.flag.p, 0, 4 * ST_WORDS, s));
        if (ev) HIPCHK(ctx, hipEventRecord(ev[2 * W3_EV_TOTAL], s));
        if ((rc = twophase_predict(ws, s, ps, d_in, n, block_size, nb, false, nullptr, ev, nullptr, ctx->err))) return rc;
        // the insurance of every encode (twophase_verify): here always before the first stage, which also covers the single leaf whose
        // stream that stage rewrites in place
        if ((rc = twophase_verify(ws, s, ps, d_in, n, block_size, nb, (uint32_t *)J.flag.p + ST_ORDER_FAULT, ctx->err))) return rc;
        StepsArgs a;
        memset(&a, 0, sizeof a);
        uint8_t *copy = (uint8_t *)ctx->steps_copies.p;
        const auto leaf_streams = ws.mix;   // (twophase_apm replaces ws.mix by its one output stream)
        for (int l = 0, k = 0; l < ps.n_leaves; l++) {
            if (leaf_class(ps.leaf[l]) == LEAF_FROZEN) continue;
            a.leaf[l] = leaf_streams.src[k++];
            if (leaf_in_P) {
                HIPCHK(ctx, hipMemcpyAsync(copy, a.leaf[l], n * 16, hipMemcpyDeviceToDevice, s));
                a.leaf[l] = (const uint4 *)copy; copy += n * 16;
            }
        }
        if (ev) HIPCHK(ctx, hipEventRecord(ev[2 * W3_EV_APM], s));
        for (int j = 0; j < ps.n_apm; j++) {
            // the chain's own stream, a stage per call: after the first one ws.P_valid is set and the next stage reads ws.P, as the chain does
            ParsedSpec one = ps;
            one.n_apm = 1; one.apm[0] = ps.apm[j];
            if ((rc = twophase_apm(ws, s, one, d_in, n, block_size, nb, nullptr, nullptr, ctx->err))) return rc;
            a.apm[j] = (const uint4 *)ws.P;
            if (j + 1 < ps.n_apm) {
                HIPCHK(ctx, hipMemcpyAsync(copy, ws.P, n * 16, hipMemcpyDeviceToDevice, s));
                a.apm[j] = (const uint4 *)copy; copy += n * 16;
            }
        }
        if (ev) HIPCHK(ctx, hipEventRecord(ev[2 * W3_EV_APM + 1], s));
        a.in = d_in; a.n = n; a.stretch = ctx->stretch; a.rows = (uint4 *)d_rows;
        a.n_leaves = lay.n_leaves; a.n_apm = lay.n_apm; a.n_cols = lay.n_cols; a.format = format; a.col_bit = lay.col_bit;
        const dim3 grid(steps_grid(steps_tiles(n), W3_STEPS_GRID_CAP));
        if (ev) HIPCHK(ctx, hipEventRecord(ev[2 * W3_EV_CODER], s));
        if (ctx->opt.tune & W3_TUNE_STEPS_DIRECT) steps_launch<false>(lay.n_cols, grid, steps_lds_bytes(lay.n_cols), s, a);
        else steps_launch<true>(lay.n_cols, grid, steps_lds_bytes(lay.n_cols), s, a);
        HIPCHK(ctx, hipGetLastError());
        if (ev) { HIPCHK(ctx, hipEventRecord(ev[2 * W3_EV_CODER + 1], s)); HIPCHK(ctx, hipEventRecord(ev[2 * W3_EV_TOTAL + 1], s)); }
        JobStatus st{};
        HIPCHK(ctx, hipMemcpyAsync(st.w, J.flag.p, sizeof st.w, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (!st.order_fault()) break;
        // the LDS-add rounds were not lane-ordered under this load: predict again with the ballot rounds, and stay on them (as encode_core does)
        if (attempt) { ctx->err = "predict streams differ from their ballot-round re-prediction even without LDS-add rounds (internal error)"; return W3_E_HIP; }
        lds_faults += st.order_fault();
        use_ballot_rounds(ctx);
    }
    ctx->timing.n_lds_faults += lds_faults;
    prof.n_lds_faults += lds_faults;
    prof.bytes_read += (uint64_t)n * (16ull * (n_live + ps.n_apm) + (lay.col_bit != W3_STEPS_NO_COL ? 1 : 0));
    prof.bytes_written += steps_rows_bytes(n, lay.n_cols);
    if (ev) {
        prof.predict_ms += elapsed_ev(ev, W3_EV_PREDICT); prof.rows_ms += elapsed_ev(ev, W3_EV_CODER); prof.total_ms += elapsed_ev(ev, W3_EV_TOTAL);
        if (ps.n_apm) prof.apm_ms += elapsed_ev(ev, W3_EV_APM);
    }
    return W3_OK;
}

// the checks both forms share, in the order include/w3hip.h gives; *go = there is something to do
static int steps_args(w3_ctx *ctx, const w3_model_spec *spec, const void *in, size_t n, size_t block_size, uint32_t format, uint32_t flags, const void *rows,
                      size_t rows_cap, bool one_device, ParsedSpec &ps, StepsLayout &lay, bool *go) {
    *go = false;
    int rc = check_args(ctx, n, block_size, one_device);
    if (rc) return rc;
    if ((rc = jobs_idle(ctx))) return rc;   // (the predict phase runs on job 0's workspace)
    if ((rc = parse_spec(spec, ps))) { ctx->err = "malformed model spec"; return rc; }
    // the row kernel recomputes the mix column with OpinionMixer2 (mix_p); a logistic mixer's column would have to come from a copy of ws.P
    if (ps.has_mix) { ctx->err = "w3_export_steps_*: specs with a logistic mixer node (W3_NODE_MIX) are not exported"; return W3_E_UNSUPPORTED; }
    if (!steps_layout((uint32_t)ps.n_leaves, (uint32_t)ps.n_apm, format, flags, lay)) { ctx->err = "unknown W3_STEPS_* format or flag"; return W3_E_INVALID; }
    memset(&ctx->steps_prof, 0, sizeof ctx->steps_prof);
    ctx->steps_prof.direct_stores = (ctx->opt.tune & W3_TUNE_STEPS_DIRECT) ? 1u : 0u;
    if (n == 0) return W3_OK;
    if (!in || !rows) return W3_E_INVALID;
    if (((uintptr_t)rows & 15u) != 0) { ctx->err = "rows must be 16-byte aligned"; return W3_E_INVALID; }
    if (rows_cap < steps_rows_bytes(n, lay.n_cols)) { ctx->err = "rows_cap too small: " + std::to_string(steps_rows_bytes(n, lay.n_cols)) + " bytes needed"; return W3_E_NOSPACE; }
    if (!twophase_supported(ps, block_size, n)) { ctx->err = "spec not covered by the two-phase predict kernels"; return W3_E_UNSUPPORTED; }
    memset(&ctx->timing, 0, sizeof ctx->timing);
    ctx->timing.path = W3_PATH_TWOPHASE; ctx->timing.n_parts = 0;
    *go = true;
    return W3_OK;
}

extern "C" int w3_export_steps_device(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *d_in, size_t n, size_t block_size, uint32_t format,
                                      uint32_t flags, void *d_rows, size_t rows_cap, void *stream) {
    ParsedSpec ps;
    StepsLayout lay;
    bool go;
    int rc = steps_args(ctx, spec, d_in, n, block_size, format, flags, d_rows, rows_cap, true, ps, lay, &go);
    if (rc || !go) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->timing.n_parts = 1;
    return steps_run(ctx, stream ? (hipStream_t)stream : ctx->stream, ps, lay, format, d_in, n, block_size, d_rows, ctx->steps_prof);
}

extern "C" int w3_export_steps_staged(w3_ctx *ctx, const w3_model_spec *spec, const uint8_t *in, size_t n, size_t block_size, uint32_t format,
                                      uint32_t flags, void *rows, size_t rows_cap) {
    ParsedSpec ps;
    StepsLayout lay;
    bool go;
    int rc = steps_args(ctx, spec, in, n, block_size, format, flags, rows, rows_cap, false, ps, lay, &go);
    if (rc || !go) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // pieces of whole blocks; a piece's rows are C x 16 bytes per input byte, so the default piece is 2 GiB of ROWS, not of input
    const uint64_t auto_blocks = std::max<uint64_t>(1, (1ull << 31) / (16ull * lay.n_cols * block_size));
    const uint64_t run_blocks = ctx->host_chunk_blocks ? (uint64_t)ctx->host_chunk_blocks : auto_blocks;
    const size_t piece = (size_t)steps_piece_len(n, block_size, run_blocks, 0);
    if (piece >= (1ull << 32) - 4096u) { ctx->err = "W3_OPT_HOST_CHUNK_BLOCKS: a piece must stay below 4 GiB of input"; return W3_E_UNSUPPORTED; }
    if (n % piece && n % piece < 8) { ctx->err = "a last piece below 8 bytes is not covered by the two-phase predict kernels"; return W3_E_UNSUPPORTED; }
    ENSURE(ctx, ctx->io_in, piece);
    ENSURE(ctx, ctx->steps_rows, (size_t)steps_rows_bytes(piece, lay.n_cols));
    VcallPin pin(ctx, verify_call(ctx, n, block_size));   // (one call, one number for the verification's rotation, whatever the pieces)
    for (size_t o0 = 0; o0 < n;) {
        const size_t len = (size_t)steps_piece_len(n, block_size, run_blocks, o0);
        HIPCHK(ctx, hipMemcpyAsync(ctx->io_in.p, in + o0, len, hipMemcpyHostToDevice, s));
        if ((rc = steps_run(ctx, s, ps, lay, format, (const uint8_t *)ctx->io_in.p, len, block_size, ctx->steps_rows.p, ctx->steps_prof))) return rc;
        HIPCHK(ctx, hipMemcpy((uint8_t *)rows + steps_rows_bytes(o0, lay.n_cols), ctx->steps_rows.p, (size_t)steps_rows_bytes(len, lay.n_cols), hipMemcpyDeviceToHost));
        ctx->timing.n_parts++;
        o0 += len;
    }
    return W3_OK;
}

extern "C" int w3_export_steps_get_profile(const w3_ctx *ctx, w3_steps_profile *out) {
    if (!ctx || !out) return W3_E_INVALID;
    *out = ctx->steps_prof;
    return W3_OK;
}

// ---------------------------------------------------------------------------
// read-only tables (host-side known-answer surface)
// ---------------------------------------------------------------------------
extern "C" int w3_state_table(uint16_t *out) {
    if (!out) return W3_E_INVALID;
    std::vector<StEntry> t(kStSize);
    build_state_table(t.data());
    for (int i = 0; i < kStSize; i++) { out[3 * i] = t[i].prob; out[3 * i + 1] = t[i].next0; out[3 * i + 2] = t[i].next1; }
    return W3_OK;
}

extern "C" int w3_stretch_squash(int16_t *stretch, uint16_t *squash) {
    if (!stretch || !squash) return W3_E_INVALID;
    build_stretch_squash(stretch, squash);
    return W3_OK;
}

// ---------------------------------------------------------------------------
// device self-test
// ---------------------------------------------------------------------------
extern "C" int w3_selftest_counter_p(w3_ctx *ctx, uint64_t *mismatches) {
    if (!ctx || !mismatches) return W3_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->total, 8);
    HIPCHK(ctx, hipMemsetAsync(ctx->total.p, 0, 8, ctx->stream));
    for (uint32_t lo = 0; lo < 65536; lo += 4096) {
        hipLaunchKernelGGL(k_selftest_counter_p, dim3(256 * 16), dim3(256), 0, ctx->stream, (unsigned long long *)ctx->total.p, lo, lo + 4096);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(mismatches, ctx->total.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return W3_OK;
}

extern "C" int w3_debug_get_stamps(w3_ctx *ctx, uint64_t out[8]) {
    if (!ctx || !out) return W3_E_INVALID;
    memset(out, 0, 64);
    if (!ctx->jobs[0].tp.dbg) return W3_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(out, ctx->jobs[0].tp.dbg, 64, hipMemcpyDeviceToHost));
    return W3_OK;
}
