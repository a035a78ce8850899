// w3_jobs.h — the decisions of the submit / wait job machinery (w3hip.hip) as pure functions of plain numbers: how many calls are kept
// in flight and how, which slot a submitted call takes, and what a call's status words ask for.  Host only, no HIP include:
// tests/host/jobs_plan.cpp compiles it with g++ and compares it with the three inline forms these rules had.
#pragma once
#include <cstdint>

namespace w3 {

// Jobs in flight: free-running — every code stage on its own stream, the calls' coders overlapping one another — while a call's
// coder leaves a good part of the chip idle: four up to W3_FREE_RUN4_BLOCKS blocks (64 coder workgroups), three up to
// W3_FREE_RUN_BLOCKS (measured: 7,629 blocks 36.6 ms per step with three, 39.1 with four, 43.8 with the ordered pair; 11,444 blocks
// 53.6 against 56.0 ordered; at 15,259 the two forms meet at 68-70 ms); beyond that the ordered pair of DESIGN.md section 3.3
// (a job workspace is ~70 bytes per input byte).
#define W3_MAX_JOBS 4
#define W3_FREE_RUN_BLOCKS 12288u
#define W3_FREE_RUN4_BLOCKS 4096u

// How submitted calls of a spec and size are kept in flight (w3_encode_submit and the *_max_in_flight entry points agree by calling this).
//   ordered pair   step k's coder beside step k+1's rank kernels, APM stage in between: large inputs of models with
//                  wide (sorted) leaves AND an APM stage — the bench model: 14,1xx MiB/s against 13,570 free-running;
//   free-running   every code stage on its own stream as soon as it is submitted: small and medium inputs of any model, and large inputs
//                  of models WITHOUT rank kernels to put the coder beside (1e9 B: Order0 38,099 -> 52,642 MiB/s with three in flight,
//                  main.rs's default model 15,578 -> 17,566; order012, wide leaves but no APM stage, 16,038 -> 16,313 with two).
// n_wide: leaves that run rank kernels; n_apm: APM stages; has_slot: a slot-state leaf; nb: blocks; tune: W3_OPT_TUNE.
struct PipelinePlan { bool free_run; int depth; };
static inline PipelinePlan pipeline_plan(int n_wide, int n_apm, bool has_slot, uint32_t nb, uint32_t tune) {
    PipelinePlan p;
    p.free_run = (nb <= W3_FREE_RUN_BLOCKS || n_wide == 0 || n_apm == 0 || (tune & 8192u)) && !(tune & 4096u);   // (W3_OPT_TUNE bit 12: ordered, 13: free-running, whatever the size)
    if (has_slot) p.depth = 2;                          // (event records: 32 bytes per input byte and leaf)
    else if (!p.free_run) p.depth = 2;
    else if (nb <= W3_FREE_RUN4_BLOCKS) p.depth = W3_MAX_JOBS;
    else if (nb <= W3_FREE_RUN_BLOCKS) p.depth = 3;
    else p.depth = n_wide == 0 ? 3 : 2;                 // large inputs: a workspace is 16 bytes per input byte and live leaf (+ 40 per wide leaf)
    return p;
}

// The slot of the next submitted call.  busy[k] != 0: slot k holds a call.  At most `depth` calls are in flight, whichever slots they
// hold (a call of another size may have taken a slot beyond this call's depth); the call takes slot next_job % depth, or, where that
// one is taken, the first free slot below depth (calls may be waited for in any order).  slot < 0: refused, in_flight says why.
// The host-buffer and sharded searches ask with next_job = 0: the first free slot.
struct SlotPick { int slot, in_flight; };
static inline SlotPick pick_slot(const int *busy, int n_slots, int next_job, int depth) {
    SlotPick p{-1, 0};
    for (int k = 0; k < n_slots; k++) p.in_flight += busy[k] != 0;
    if (p.in_flight >= depth) return p;
    int j = next_job % depth;
    if (busy[j])
        for (int k = 0; k < depth && k < n_slots; k++)
            if (!busy[k]) { j = k; break; }
    if (!busy[j]) p.slot = j;
    return p;
}

// The status words of one encode: a device buffer the kernels write, read back when the call's kernels are through.
enum { ST_FLAGS = 0 /* ST_F_* */, ST_HANDED_BACK = 1 /* blocks the fast coder gave up on (pending-bit run beyond its accumulator) */,
       ST_ORDER_FAULT = 2 /* waves whose LDS-add rounds differ from their ballot-round re-prediction (twophase_verify) */,
       ST_APM_OOB = 3 /* -DW3_TUNING builds: APM stores outside the stage's stream and the sink */, ST_WORDS = 4 };
enum : uint32_t { ST_F_OVERFLOW = 1u /* a block outgrew its stripe */, ST_F_TIMEOUT = 2u /* the coder pipeline gave up waiting */ };
struct JobStatus {
    uint32_t w[ST_WORDS];
    bool overflow() const { return (w[ST_FLAGS] & ST_F_OVERFLOW) != 0; }
    bool timeout() const { return (w[ST_FLAGS] & ST_F_TIMEOUT) != 0; }
    uint32_t handed_back() const { return w[ST_HANDED_BACK]; }
    uint32_t order_fault() const { return w[ST_ORDER_FAULT]; }
    uint32_t apm_oob() const { return w[ST_APM_OOB]; }
};

// What the status words of an attempt ask for.  cap_raised: the stripes already have the worst-case size; fault_seen: an earlier attempt
// of this call already fell back to the ballot rounds; two_phase: the call ran the two-phase path (only it hands blocks back or verifies).
enum JobAction {
    JOB_DONE,
    JOB_BALLOT_ROUNDS,   // the LDS-add rounds were not lane-ordered under this load: the streams cannot be trusted, code the call again with
                         // the ballot rounds and keep the context on them.  Before everything else: the other words describe those streams
    JOB_RECODE,          // code the handed-back blocks with the careful coder, read the status again, then job_classify_coded
    JOB_RAISE_CAP,       // rare: a block expanded past 2N+64: again with the worst-case stripes
    JOB_ERR_ORDER_FAULT, JOB_ERR_TIMEOUT, JOB_ERR_APM_OOB, JOB_ERR_OVERFLOW   // internal errors
};
// (what is left to ask once the streams are trusted and nothing is handed back)
static inline JobAction job_classify_coded(const JobStatus &s, bool cap_raised) {
    if (s.timeout()) return JOB_ERR_TIMEOUT;
    if (s.apm_oob()) return JOB_ERR_APM_OOB;
    if (!s.overflow()) return JOB_DONE;
    return cap_raised ? JOB_ERR_OVERFLOW : JOB_RAISE_CAP;
}
static inline JobAction job_classify(const JobStatus &s, bool cap_raised, bool fault_seen, bool two_phase) {
    if (two_phase && s.order_fault()) return fault_seen ? JOB_ERR_ORDER_FAULT : JOB_BALLOT_ROUNDS;
    if (two_phase && s.handed_back()) return JOB_RECODE;
    return job_classify_coded(s, cap_raised);
}
// w3_encode_wait does not repair a finished job in place: anything but done or an internal error is run again, synchronously and alone
// (encode_core's retry loop then takes each action in turn), and an internal error the words already show is reported at once.
static inline JobAction job_classify_waited(const JobStatus &s) {
    if (s.timeout() && !s.order_fault()) return JOB_ERR_TIMEOUT;
    if (s.apm_oob()) return JOB_ERR_APM_OOB;
    if (s.order_fault()) return JOB_BALLOT_ROUNDS;
    if (s.handed_back()) return JOB_RECODE;
    return s.overflow() ? JOB_RAISE_CAP : JOB_DONE;
}

}   // namespace w3
