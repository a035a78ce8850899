// The decisions of the submit / wait job machinery (weath3rb0i_amd/csrc/w3_jobs.h) against the inline forms they had in w3hip.hip,
// spelled out here as they stood: the pipeline plan, the three slot searches, and the two readings of a call's status words.
// Usage: jobs_plan [rounds]   (seeded; prints "jobs plan ok", or FAIL lines on stderr and exit status 1)
#include "../../weath3rb0i_amd/csrc/w3_jobs.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace w3;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// ---- the plan, as w3hip.hip's pipeline_plan had it (constants included) ----
static void old_plan(int n_wide, int n_apm, bool has_slot, uint32_t nb, uint32_t tune, bool &free_run, int &depth) {
    free_run = (nb <= 12288u || n_wide == 0 || n_apm == 0 || (tune & 8192u)) && !(tune & 4096u);
    if (has_slot) depth = 2;
    else if (!free_run) depth = 2;
    else if (nb <= 4096u) depth = 4;
    else if (nb <= 12288u) depth = 3;
    else depth = n_wide == 0 ? 3 : 2;
}

static void check_plan(int n_wide, int n_apm, bool has_slot, uint32_t nb, uint32_t tune) {
    bool fr; int d;
    old_plan(n_wide, n_apm, has_slot, nb, tune, fr, d);
    const PipelinePlan p = pipeline_plan(n_wide, n_apm, has_slot, nb, tune);
    CHECK(p.free_run == fr && p.depth == d, "wide %d apm %d slot %d nb %u tune %u: {%d, %d}, was {%d, %d}", n_wide, n_apm, has_slot, nb, tune, p.free_run, p.depth, fr, d);
    CHECK(p.depth >= 2 && p.depth <= W3_MAX_JOBS, "depth %d", p.depth);
    if (has_slot) CHECK(p.depth == 2, "slot leaves: depth %d (nb %u tune %u)", p.depth, nb, tune);
    if (!p.free_run) CHECK(p.depth == 2, "ordered: depth %d (nb %u tune %u)", p.depth, nb, tune);
}

// ---- the slot searches, as they stood ----
// w3_encode_submit: states of the W3_MAX_JOBS device slots
static int old_device_slot(const int *state, int next_job, int depth, int &in_flight) {
    in_flight = 0;
    for (int k = 0; k < W3_MAX_JOBS; k++) in_flight += state[k] != 0;
    int j = next_job % depth;
    if (state[j] != 0) {
        for (int k = 0; k < depth; k++)
            if (state[k] == 0) { j = k; break; }
    }
    if (in_flight >= depth || state[j] != 0) return -1;
    return j;
}
// host_submit_core (n_slots = W3_MAX_JOBS + 1) and, with state[k] = "some context holds a shard in slot k", w3_encode_sharded_submit
static int old_first_free_slot(const int *state, int n_slots, int depth, int &busy) {
    busy = 0;
    int slot = -1;
    for (int k = 0; k < n_slots; k++) {
        if (state[k] != 0) busy++;
        else if (slot < 0) slot = k;
    }
    if (busy >= depth || slot < 0) return -1;
    return slot;
}

// ---- the status words, as encode_core's retry loop read them: the first thing it did ----
static JobAction old_loop_action(const uint32_t fl[4], bool cap_raised, bool fault_seen, bool two) {
    if (two && fl[2]) return fault_seen ? JOB_ERR_ORDER_FAULT : JOB_BALLOT_ROUNDS;
    if (two && fl[1]) return JOB_RECODE;   // (then the words were read again and the loop went on below)
    if (fl[0] & 2u) return JOB_ERR_TIMEOUT;
    if (fl[3]) return JOB_ERR_APM_OOB;
    if (!(fl[0] & 1u)) return JOB_DONE;
    if (cap_raised) return JOB_ERR_OVERFLOW;
    return JOB_RAISE_CAP;
}
// ... what it did with the words read again after a recode
static JobAction old_loop_after_recode(const uint32_t fl[4], bool cap_raised) {
    if (fl[0] & 2u) return JOB_ERR_TIMEOUT;
    if (fl[3]) return JOB_ERR_APM_OOB;
    if (!(fl[0] & 1u)) return JOB_DONE;
    if (cap_raised) return JOB_ERR_OVERFLOW;
    return JOB_RAISE_CAP;
}
// ... and as w3_encode_wait read them: 0 done, 1 timeout error, 2 store-guard error, 3 run again, 4 run again on the ballot rounds
static int old_wait_action(const uint32_t h_status[4]) {
    const uint32_t f0 = h_status[0], redo = h_status[1], mism = h_status[2];
    if ((f0 & 2u) && !mism) return 1;
    if (h_status[3]) return 2;
    if (f0 || redo || mism) return mism ? 4 : 3;
    return 0;
}
static int wait_action_of(JobAction a) {
    switch (a) {
    case JOB_DONE: return 0;
    case JOB_ERR_TIMEOUT: return 1;
    case JOB_ERR_APM_OOB: return 2;
    case JOB_BALLOT_ROUNDS: return 4;
    default: return 3;   // (w3_encode_wait's switch: everything else runs the call again)
    }
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 400;
    std::mt19937_64 rng(0x6a6f6273u);

    // the plan: the edges, every leaf combination, the two tune bits alone and together (and beside other bits)
    const uint32_t nbs[] = {0u, 1u, 4096u, 4097u, 12288u, 12289u, 0xFFFFFFFFu};
    const uint32_t tunes[] = {0u, 4096u, 8192u, 4096u | 8192u, 0xFFFFFu & ~(4096u | 8192u), 0xFFFFFu};
    for (uint32_t nb : nbs)
        for (int n_wide : {0, 1, 3})
            for (int n_apm : {0, 1})
                for (int has_slot = 0; has_slot < 2; has_slot++)
                    for (uint32_t tune : tunes) check_plan(n_wide, n_apm, has_slot != 0, nb, tune);
    for (int it = 0; it < rounds * 100; it++) {
        const uint32_t r = (uint32_t)rng();
        const uint32_t nb = (r & 3u) == 0 ? (uint32_t)rng() : (uint32_t)(rng() % 20000u);
        check_plan((int)(rng() % 5u), (int)(rng() % 3u), (rng() & 1u) != 0, nb, (uint32_t)rng() & 0xFFFFFu);
    }

    // the slot searches over random submit / wait sequences, waits in any order, the depth changing from call to call
    for (int it = 0; it < rounds; it++) {
        for (int n_slots : {W3_MAX_JOBS, W3_MAX_JOBS + 1}) {
            std::vector<int> state(n_slots, 0);
            int next_job = 0;
            for (int step = 0; step < 200; step++) {
                if (rng() % 3u == 0) {   // a wait, for any slot that holds a call
                    std::vector<int> held;
                    for (int k = 0; k < n_slots; k++) if (state[k]) held.push_back(k);
                    if (!held.empty()) state[held[rng() % held.size()]] = 0;
                    continue;
                }
                const int depth = 2 + (int)(rng() % (uint32_t)(n_slots - 1));   // [2, n_slots]
                int in_flight = 0;
                for (int k = 0; k < n_slots; k++) in_flight += state[k] != 0;
                const bool first_free = n_slots != W3_MAX_JOBS || (rng() & 1u);   // the host and sharded searches: next_job = 0
                const SlotPick p = pick_slot(state.data(), n_slots, first_free ? 0 : next_job, depth);
                CHECK(p.in_flight == in_flight, "in flight %d, counted %d", p.in_flight, in_flight);
                CHECK((p.slot < 0) == (in_flight >= depth), "slot %d with %d in flight at depth %d", p.slot, in_flight, depth);
                if (p.slot >= 0) {
                    CHECK(p.slot < n_slots && state[p.slot] == 0, "slot %d is taken", p.slot);
                    if (p.slot >= n_slots || state[p.slot] != 0) break;
                }
                int was_count = 0;
                const int was = first_free ? old_first_free_slot(state.data(), n_slots, depth, was_count) : old_device_slot(state.data(), next_job, depth, was_count);
                CHECK(p.slot == was && p.in_flight == was_count, "slot %d (%d in flight), was %d (%d): next %d depth %d", p.slot, p.in_flight, was, was_count, next_job, depth);
                if (p.slot >= 0) {
                    if (!first_free && state[next_job % depth] == 0) CHECK(p.slot == next_job % depth, "slot %d, %d was free", p.slot, next_job % depth);
                    state[p.slot] = 1 + (int)(rng() % 3u);   // (the states a slot goes through: all that matters is non-zero)
                    next_job = p.slot + 1;
                }
            }
        }
    }

    // the status words: every zero / non-zero combination of the five signals (a non-zero count takes two values: nothing may depend on
    // which) x cap_raised x fault_seen x two_phase
    for (uint32_t m = 0; m < 32u; m++)
        for (uint32_t big = 0; big < 2u; big++) {
            const uint32_t c = big ? 0x80000001u : 1u;
            JobStatus s{};
            s.w[ST_FLAGS] = ((m & 1u) ? ST_F_OVERFLOW : 0u) | ((m & 2u) ? ST_F_TIMEOUT : 0u);
            s.w[ST_HANDED_BACK] = (m & 4u) ? c : 0u; s.w[ST_ORDER_FAULT] = (m & 8u) ? c : 0u; s.w[ST_APM_OOB] = (m & 16u) ? c : 0u;
            const uint32_t fl[4] = {((m & 1u) ? 1u : 0u) | ((m & 2u) ? 2u : 0u), (m & 4u) ? c : 0u, (m & 8u) ? c : 0u, (m & 16u) ? c : 0u};
            for (int k = 0; k < 4; k++) CHECK(s.w[k] == fl[k], "word %d: the enumerators moved (%u, was %u)", k, s.w[k], fl[k]);
            for (int f = 0; f < 8; f++) {
                const bool cap_raised = f & 1, fault_seen = (f & 2) != 0, two = (f & 4) != 0;
                const JobAction a = job_classify(s, cap_raised, fault_seen, two), was = old_loop_action(fl, cap_raised, fault_seen, two);
                CHECK(a == was, "signals %u cap_raised %d fault_seen %d two %d: action %d, the loop took %d", m, cap_raised, fault_seen, two, (int)a, (int)was);
                CHECK(job_classify_coded(s, cap_raised) == old_loop_after_recode(fl, cap_raised), "signals %u cap_raised %d after a recode", m, cap_raised);
            }
            const int w = wait_action_of(job_classify_waited(s)), w_was = old_wait_action(fl);   // (what w3_encode_wait sees: a first attempt of a two-phase call)
            CHECK(w == w_was, "signals %u: w3_encode_wait does %d, did %d", m, w, w_was);
        }

    if (fails) { fprintf(stderr, "FAIL: %d checks\n", fails); return 1; }
    printf("jobs plan ok\n");
    return 0;
}
