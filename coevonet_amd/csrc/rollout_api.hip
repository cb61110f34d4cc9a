// coevo_mpe_rollout - a whole batch of games in ONE C-ABI call: the replacement for the reference's per-game
// play_game()/play_MPE() loop (utils/game_logic_functions.py:123-228) at batch scale.
//
// Per env-cycle and cohort it enqueues ONE merged launch (coevo_mpe_policy_cycle_merged: shared-opponent workgroups on
// the matrix cores + per-individual streaming workgroups, env step fused in); cohorts are independent chains on their
// own streams (cohort 0: the caller's).  With d->merged == 0 the older two-launch form is used instead: [side stream]
// the shared-opponent launch || [main stream] the per-individual launch, joined by an event.  Nothing here synchronises
// with the host; a single-cohort sequence can also be captured into a hipGraph by the caller.
// coevo_mpe16_rollout plays an fp16 slab through the same driver (enqueue_rollout below) with its own per-cycle launcher.
#include <cstdlib>
#include <vector>

#include "coevo_common.hip.h"

static_assert(sizeof(coevo_rollout_desc) == 192, "layout mirrored by coevonet_amd/lib.py RolloutDesc");

__global__ void stamps_init_kernel(uint64_t *stamps, int n)
{
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        stamps[2 * i] = ~0ull;
        stamps[2 * i + 1] = 0ull;
    }
}

// stream of one cohort beyond the first (the first cohort uses the caller's stream)
struct cohort_lane {
    hipStream_t s = nullptr;
    hipEvent_t done = nullptr;
};

struct coevo_rollout_ctx {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr, start = nullptr;
    std::vector<cohort_lane> lanes;  // created on first use
    std::vector<hipEvent_t> timing;  // pairs (start, end) around the light launch of each cycle
    int pairs_used = 0;
};

extern "C" void *coevo_rollout_ctx_create(int n_timing_pairs)
{
    auto *c = new coevo_rollout_ctx();
    int prio_lo = 0, prio_hi = 0;  // numerically lowest = highest priority
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->start, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return nullptr;
    }
    c->timing.resize(2 * (size_t)(n_timing_pairs > 0 ? n_timing_pairs : 0));
    for (auto &e : c->timing)
        if (hipEventCreate(&e) != hipSuccess) { delete c; return nullptr; }
    return c;
}

extern "C" void coevo_rollout_ctx_destroy(void *ctx)
{
    auto *c = static_cast<coevo_rollout_ctx *>(ctx);
    if (!c) return;
    for (auto e : c->timing) (void)hipEventDestroy(e);
    for (auto &ln : c->lanes) {
        if (ln.done) (void)hipEventDestroy(ln.done);
        if (ln.s) (void)hipStreamDestroy(ln.s);
    }
    if (c->start) (void)hipEventDestroy(c->start);
    if (c->fork) (void)hipEventDestroy(c->fork);
    if (c->join) (void)hipEventDestroy(c->join);
    if (c->side) (void)hipStreamDestroy(c->side);
    delete c;
}

// streams for up to n_cohorts independent cohorts (coevo_rollout_desc.n_cohorts); call outside graph capture
extern "C" int coevo_rollout_ctx_reserve_cohorts(void *ctx, int n_cohorts)
{
    auto *c = static_cast<coevo_rollout_ctx *>(ctx);
    if (!c || n_cohorts < 1 || n_cohorts > COEVO_MAX_COHORTS) return COEVO_ERR_ARG;
    while ((int)c->lanes.size() < n_cohorts - 1) {
        cohort_lane ln;
        if (hipStreamCreateWithFlags(&ln.s, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ln.done, hipEventDisableTiming) != hipSuccess)
            return COEVO_ERR_HIP;
        c->lanes.push_back(ln);
    }
    return COEVO_OK;
}

// the stream cohort k (>= 1) of this context runs on (cohort 0 runs on the caller's stream): for callers that enqueue
// per-cohort work (breeding, resets) in front of a cohort's chain themselves
extern "C" void *coevo_rollout_ctx_cohort_stream(void *ctx, int k)
{
    auto *c = static_cast<coevo_rollout_ctx *>(ctx);
    if (!c || k < 1 || k > (int)c->lanes.size()) return nullptr;
    return c->lanes[k - 1].s;
}

// generic use of the context's timing event pairs: bracket whatever is enqueued on `stream` between the two calls (eager
// enqueue only - events cannot be recorded inside a captured graph on this runtime); read with
// coevo_rollout_ctx_light_times.  Used by coevo_dqn_forward_argmax_timed around its dominant kernel.
extern "C" int coevo_timing_begin(void *ctx, void *stream)
{
    auto *c = static_cast<coevo_rollout_ctx *>(ctx);
    if (!c) return COEVO_ERR_ARG;
    if (2 * (size_t)c->pairs_used + 1 >= c->timing.size()) return COEVO_OK;   // out of pairs: stop sampling, keep running
    COEVO_HIP_CHECK(hipEventRecord(c->timing[2 * c->pairs_used], (hipStream_t)stream));
    return COEVO_OK;
}

extern "C" int coevo_timing_end(void *ctx, void *stream)
{
    auto *c = static_cast<coevo_rollout_ctx *>(ctx);
    if (!c) return COEVO_ERR_ARG;
    if (2 * (size_t)c->pairs_used + 1 >= c->timing.size()) return COEVO_OK;
    COEVO_HIP_CHECK(hipEventRecord(c->timing[2 * c->pairs_used + 1], (hipStream_t)stream));
    c->pairs_used += 1;
    return COEVO_OK;
}

extern "C" int coevo_rollout_ctx_reset_timing(void *ctx)
{
    auto *c = static_cast<coevo_rollout_ctx *>(ctx);
    if (!c) return COEVO_ERR_ARG;
    c->pairs_used = 0;
    return COEVO_OK;
}

// elapsed milliseconds of every timed light launch so far (blocks until they have completed); returns the count
extern "C" int coevo_rollout_ctx_light_times(void *ctx, float *ms_out, int max_out)
{
    auto *c = static_cast<coevo_rollout_ctx *>(ctx);
    if (!c || !ms_out) return COEVO_ERR_ARG;
    int n = c->pairs_used < max_out ? c->pairs_used : max_out;
    for (int i = 0; i < n; ++i) {
        if (hipEventSynchronize(c->timing[2 * i + 1]) != hipSuccess) return COEVO_ERR_HIP;
        if (hipEventElapsedTime(&ms_out[i], c->timing[2 * i], c->timing[2 * i + 1]) != hipSuccess) return COEVO_ERR_HIP;
    }
    return n;
}

// ---------------------------------------------------------------------------------------------------------------------
// The rollout driver.  coevo_mpe_rollout and coevo_mpe16_rollout are enqueue_rollout() with their own per-cycle launcher;
// everything a descriptor means apart from "launch cycle c of cohort k" is written here, once.

static int cohort_count(const coevo_rollout_desc *d) { return d->n_cohorts > 1 ? d->n_cohorts : 1; }

// The buffer-parity rule (coevo.h, coevo_rollout_desc): state buffer 0 (d->state) holds the reset state, cycle c derives its
// state from the one cycle c-1 left and its owner rows write it to buffer c & 1 (d->state_alt is buffer 1) - except cycle 0,
// which plays on the reset state and writes none; every cycle writes its actions to action buffer c & 1.
// So the state AND the actions that cycle c left are in buffer buffer_after(c); c = n_cycles - 1 is what the closing step
// reads (-1: no cycle ran, the reset state).
static int buffer_after(int cycle) { return cycle <= 0 ? 0 : cycle & 1; }
static double *state_buffer(const coevo_rollout_desc *d, int b) { return b ? d->state_alt : d->state; }
static int32_t *action_buffer(const coevo_rollout_desc *d, int b)
{
    return d->actions_by_game ? d->actions_by_game + (size_t)b * 3 * (size_t)d->n_games : nullptr;   // null: unfused step
}

struct cycle_buffers {
    const double *st_prev;
    double *st_next;
    const int32_t *act_prev;
    int32_t *act_cur;
};

static cycle_buffers buffers_of_cycle(const coevo_rollout_desc *d, int cyc)
{
    // (cycle 0 never writes st_next: it only has to differ from st_prev)
    return {state_buffer(d, buffer_after(cyc - 1)), state_buffer(d, cyc == 0 ? 1 : cyc & 1), action_buffer(d, (cyc + 1) & 1),
            action_buffer(d, cyc & 1)};
}

// [n_cohorts][n_cycles][COEVO_STAMP_SLOTS][2]
static uint64_t *stamps_of(const coevo_rollout_desc *d, int k, int cyc)
{
    return d->light_stamps ? d->light_stamps + 2 * COEVO_STAMP_SLOTS * ((size_t)k * d->n_cycles + cyc) : nullptr;
}

// [n_cohorts][coevo_mpe_persistent_sync_words(n_games)]
static int32_t *sync_words_of(const coevo_rollout_desc *d, int k)
{
    return d->sync_words + (size_t)k * (size_t)coevo_mpe_persistent_sync_words(d->n_games);
}

// Every refusal of both entry points, in front of every launch.  fp16: the float16 entry has the fused env step only and no
// persistent form.
static int refuse(const coevo_rollout_desc *d, const coevo_rollout_ctx *c, bool fp16)
{
    if (!d || !d->slab || !d->state || !d->row_game || !d->row_slot || !d->status) return COEVO_ERR_ARG;
    if (fp16 ? (!d->state_alt || !d->actions_by_game) : ((d->state_alt == nullptr) != (d->actions_by_game == nullptr)))
        return COEVO_ERR_ARG;
    if (!d->state_alt && (!d->game_rows || !d->actions)) return COEVO_ERR_ARG;
    if (d->n_games <= 0 || d->n_cycles < 0 || d->n_heavy < 0 || d->n_light < 0) return COEVO_ERR_ARG;
    if ((d->n_heavy > 0 && !d->heavy) || (d->n_light > 0 && !d->light)) return COEVO_ERR_ARG;
    if (fp16 && d->sync_words) return COEVO_ERR_UNSUPPORTED;
    const int K = cohort_count(d);
    if (K == 1) return COEVO_OK;
    if (!c || !d->state_alt || !d->heavy_begin || !d->light_begin || K > COEVO_MAX_COHORTS) return COEVO_ERR_ARG;
    if (d->heavy_begin[0] != 0 || d->light_begin[0] != 0 || d->heavy_begin[K] != d->n_heavy || d->light_begin[K] != d->n_light)
        return COEVO_ERR_ARG;
    for (int k = 0; k < K; ++k)
        if (d->heavy_begin[k + 1] < d->heavy_begin[k] || d->light_begin[k + 1] < d->light_begin[k]) return COEVO_ERR_ARG;
    // the lanes must exist already: streams cannot be created while the caller is capturing a graph
    return (int)c->lanes.size() < K - 1 ? COEVO_ERR_ARG : COEVO_OK;
}

// one cohort's share of the task tables and the stream its chain of cycles runs on
struct cohort {
    int k, K;
    const coevo_fc_task *heavy;
    int n_heavy;
    const coevo_fc_task *light;
    int n_light;
    hipStream_t s;
};

// what a per-cycle launcher answers besides an error (< 0)
enum { CYCLE_ENQUEUED = 0, COHORT_PLAYED = 1, ROLLOUT_CLOSED = 2 };

// launch_cycle(cohort, cycle, its buffers, its stamps) enqueues ONE env-cycle of one cohort on cohort.s.  It may answer
// COHORT_PLAYED (its launch plays every remaining cycle of the cohort) or ROLLOUT_CLOSED (and closed the books as well).
// A template, not a function pointer: the pipelined trainers enqueue K x n_cycles launches per generation eagerly.
template <class LaunchCycle>
static int enqueue_rollout(const coevo_rollout_desc *d, coevo_rollout_ctx *c, hipStream_t main_s, bool fp16,
                           LaunchCycle &&launch_cycle)
{
    const int bad = refuse(d, c, fp16);
    if (bad) return bad;
    const int K = cohort_count(d);
    if (d->light_stamps && d->n_cycles > 0 && !d->stamps_armed) {  // {UINT64_MAX, 0}, re-armed by every enqueue / replay
        hipLaunchKernelGGL(stamps_init_kernel, dim3(1), dim3(256), 0, main_s, d->light_stamps,
                           K * d->n_cycles * COEVO_STAMP_SLOTS);
        COEVO_HIP_CHECK(hipGetLastError());
    }
    if (K > 1) {
        // One stream per cohort, forked from / joined to the caller's stream only.  (Under graph capture this runtime
        // tolerates mutual waits between the origin stream and a forked stream - the two-launch pair of coevo_mpe_rollout -
        // but two forked streams that wait on each other send hip::Stream::EndCapture into endless recursion.)  Inside a
        // cohort the launches of a cycle therefore run back to back; the overlap of matrix-core work with weight
        // streaming comes from the other cohorts' launches.
        COEVO_HIP_CHECK(hipEventRecord(c->start, main_s));
        for (int k = 1; k < K; ++k) COEVO_HIP_CHECK(hipStreamWaitEvent(c->lanes[k - 1].s, c->start, 0));
    }
    bool closed = false;
    for (int k = 0; k < K; ++k) {   // enqueue order = cohort by cohort; the chains only meet again at the `done` events
        const int hb = K > 1 ? d->heavy_begin[k] : 0, he = K > 1 ? d->heavy_begin[k + 1] : d->n_heavy;
        const int lb = K > 1 ? d->light_begin[k] : 0, le = K > 1 ? d->light_begin[k + 1] : d->n_light;
        const cohort co{k, K, d->heavy ? d->heavy + hb : nullptr, he - hb, d->light ? d->light + lb : nullptr, le - lb,
                        k ? c->lanes[k - 1].s : main_s};
        for (int cyc = 0; cyc < d->n_cycles; ++cyc) {
            const int rc = launch_cycle(co, cyc, buffers_of_cycle(d, cyc), stamps_of(d, k, cyc));
            if (rc < 0) return rc;
            closed |= rc == ROLLOUT_CLOSED;
            if (rc != CYCLE_ENQUEUED) break;
        }
    }
    for (int k = 1; k < K; ++k) {
        COEVO_HIP_CHECK(hipEventRecord(c->lanes[k - 1].done, c->lanes[k - 1].s));
        COEVO_HIP_CHECK(hipStreamWaitEvent(main_s, c->lanes[k - 1].done, 0));
    }
    // the closing step; without rewards the caller closes the rollout itself (coevo_mpe_final_step), e.g. after several
    // per-cohort calls on different streams
    if (!d->rewards || closed) return COEVO_OK;
    if (!d->state_alt) return coevo_mpe_rewards(d->state, d->n_games, d->rewards, main_s);
    const int last = d->n_cycles - 1;   // -1: no cycle ran, the books are the reset state's zeros
    const double *st_last = state_buffer(d, buffer_after(last));
    const int32_t *act_last = action_buffer(d, buffer_after(last));
    if (d->pack)
        return coevo_mpe_final_step_pack(st_last, d->n_games, act_last, last, d->game_limit, d->pos_first, d->rewards,
                                         d->pack->out, d->pack->dist, d->pack->n_roles, d->pack->n_local, d->pack->hof,
                                         d->pack->dist_pitch, d->pack->dist_first, main_s);
    return coevo_mpe_final_step(st_last, d->n_games, act_last, last, d->game_limit, d->pos_first, d->rewards, main_s);
}

// HIP events cannot be read back from inside a captured graph (external event-record nodes are rejected by this runtime), so
// the event bracket (coevo_timing_begin / _end) is for eager enqueues of a single-cohort rollout only; graph replays use the
// kernels' own clock stamps instead
static bool event_timed(const cohort &co, const coevo_rollout_ctx *c, int time_light) { return co.K == 1 && time_light && c; }

extern "C" int coevo_mpe_rollout(const coevo_rollout_desc *d, void *ctx, int time_light, void *stream)
{
    auto *c = static_cast<coevo_rollout_ctx *>(ctx);
    static const char *const persistent_env = getenv("COEVO_PERSISTENT");
    static const bool persistent_ok = !(persistent_env && persistent_env[0] == '0');   // A/B
    return enqueue_rollout(d, c, (hipStream_t)stream, false,
                           [=](const cohort &co, int cyc, const cycle_buffers &b, uint64_t *stamps) -> int {
        const bool fused = d->state_alt != nullptr;
        const int conc = d->concurrent_hint > co.K ? d->concurrent_hint : co.K;
        hipStream_t ls = co.s;
        // a cohort whose workgroups are all resident at once (coevo_mpe_persistent_fits): its n_cycles as ONE persistent launch
        if (cyc == 0 && persistent_ok && fused && d->merged && d->sync_words && co.n_heavy + co.n_light > 0 &&
            coevo_mpe_persistent_fits(co.n_heavy, co.n_light, d->heavy_max_rows, d->light_max_rows, conc) == 1) {
            // one cohort = every game of the call: its launch closes the books too
            const bool closes = co.K == 1 && d->rewards != nullptr;
            const int rc = coevo_mpe_rollout_persistent(
                d->slab, co.heavy, co.n_heavy, co.light, co.n_light, d->light_max_rows, d->heavy_max_rows, d->state, d->state_alt,
                d->n_games, d->row_game, d->row_slot, d->actions_by_game, d->game_limit, d->n_cycles, d->pos_first, d->status,
                stamps, sync_words_of(d, co.k), conc, closes ? d->rewards : nullptr, closes ? d->pack : nullptr,
                d->sync_cleared, ls);
            return rc ? rc : closes ? ROLLOUT_CLOSED : COHORT_PLAYED;
        }
        if (fused && d->merged && co.n_heavy > 0 && co.n_light > 0 && d->light_max_rows <= 8)
            return coevo_mpe_policy_cycle_merged(d->slab, co.heavy, co.n_heavy, co.light, co.n_light, d->light_max_rows, b.st_prev,
                                                 b.st_next, d->n_games, d->row_game, d->row_slot, b.act_prev, b.act_cur,
                                                 d->game_limit, cyc, d->pos_first, d->status, stamps, conc, d->heavy_max_rows, ls);
        // the two-launch form: [side stream] the shared-opponent launch || [ls] the per-individual launch, joined by an event
        // (a single cohort with a context only; otherwise back to back on ls)
        const bool two = co.K == 1 && c && c->side != ls && co.n_heavy > 0 && co.n_light > 0;
        hipStream_t hs = two ? c->side : ls;
        auto policy = [&](const coevo_fc_task *tasks, int n_tasks, int max_rows, uint64_t *st, hipStream_t s) {
            if (fused)
                return coevo_mpe_policy_cycle_fused(d->slab, tasks, n_tasks, max_rows, b.st_prev, b.st_next, d->n_games,
                                                    d->row_game, d->row_slot, b.act_prev, b.act_cur, d->game_limit, cyc,
                                                    d->pos_first, d->status, st, s);
            return coevo_mpe_policy_cycle_stamped(d->slab, tasks, n_tasks, max_rows, d->state, d->n_games, d->row_game,
                                                  d->row_slot, d->actions, d->status, st, s);
        };
        int rc;
        if (two) {
            COEVO_HIP_CHECK(hipEventRecord(c->fork, ls));
            COEVO_HIP_CHECK(hipStreamWaitEvent(hs, c->fork, 0));
        }
        if (co.n_heavy > 0) {
            rc = policy(co.heavy, co.n_heavy, d->heavy_max_rows, nullptr, hs);
            if (rc) return rc;
            if (two) COEVO_HIP_CHECK(hipEventRecord(c->join, hs));
        }
        if (co.n_light > 0) {
            const bool timed = event_timed(co, c, time_light);
            if (timed && (rc = coevo_timing_begin(c, ls))) return rc;
            rc = policy(co.light, co.n_light, d->light_max_rows, stamps, ls);
            if (rc) return rc;
            if (timed && (rc = coevo_timing_end(c, ls))) return rc;
        }
        if (two) COEVO_HIP_CHECK(hipStreamWaitEvent(ls, c->join, 0));
        if (!fused) return coevo_mpe_step(d->state, d->n_games, d->game_rows, d->actions, cyc, d->game_limit, d->pos_first, ls);
        return CYCLE_ENQUEUED;
    });
}

namespace coevo {
// csrc/fc16_rollout.hip: both task tables of one cohort's env-cycle in ONE launch of the fp16 cycle kernel
int launch_fc16_cycle(const void *slab, const coevo_fc_task *heavy, int n_heavy, const coevo_fc_task *light, int n_light,
                      const double *state_prev, double *state_next, int n_games, const int32_t *row_game,
                      const int32_t *row_slot, const int32_t *act_prev, int32_t *act_cur, const int32_t *game_limit, int cycle,
                      int pos_first, int32_t *status, uint64_t *stamps, hipStream_t s);
}

// coevo_mpe_rollout for an fp16 slab: the fused env step only, one launch per env-cycle and cohort, no persistent form
extern "C" int coevo_mpe16_rollout(const coevo_rollout_desc *d, void *ctx, int time_light, void *stream)
{
    auto *c = static_cast<coevo_rollout_ctx *>(ctx);
    return enqueue_rollout(d, c, (hipStream_t)stream, true,
                           [=](const cohort &co, int cyc, const cycle_buffers &b, uint64_t *stamps) -> int {
        const bool timed = event_timed(co, c, time_light);
        int rc;
        if (timed && (rc = coevo_timing_begin(c, co.s))) return rc;
        rc = coevo::launch_fc16_cycle(d->slab, co.heavy, co.n_heavy, co.light, co.n_light, b.st_prev, b.st_next, d->n_games,
                                      d->row_game, d->row_slot, b.act_prev, b.act_cur, d->game_limit, cyc, d->pos_first,
                                      d->status, stamps, co.s);
        if (rc) return rc;
        return timed ? coevo_timing_end(c, co.s) : CYCLE_ENQUEUED;
    });
}

COEVO_DEFINE_TU_FLAGS(rollout_api)
