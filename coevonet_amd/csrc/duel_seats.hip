// Paddle duel with a scripted seat on one parity (include/coevo_duel_seats.h states the contract): the env-step launch that books
// the net's agent-step t - 1 also plays the seat's agent-step t - its action is a few integer operations on the state words
// thread 0 already holds - and renders the net's frame of step t + 1.  Three launches (conv stack, fc1, this one) per TWO
// agent-steps.  The rules, the serve, the world step and the render loop are duel_pieces.hip.h's, shared with duel_env.hip;
// scripted_action is baseline_pieces.hip.h's.
//
// Phases of a workgroup:  (1) [fused forms] output row of the net's step t-1 -> action;  (2) thread 0 loads the 16 state words
// into registers, books the net's action, takes and books the seat's action, stores the words back once, and publishes the four
// history snapshots and "render" through LDS;  barrier;  (3) all threads render the frame of step t+1 in 16-byte stores.  No
// atomics on any path a valid call takes (a faulted output row and an invalid seat raise their status bit with atomicOr).
#include "dqn_common.hip.h"
#include "dqn16_layout.hip.h"
#include "duel_pieces.hip.h"
#include "baseline_pieces.hip.h"
#include "../../include/coevo_duel_seats.h"

namespace coevo {

// one game's 16 state words in registers (coevo_duel.h's order)
struct DuelRegs {
    int pending, bx, by, vx, vy, p0, p1, s0, s1, cum0, cum1, ended;
    uint32_t h0, h1, h2, h3;
};

__device__ __forceinline__ DuelRegs duel_load(const int32_t *st)
{
    return {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], st[9], st[10], st[11],
            (uint32_t)st[12], (uint32_t)st[13], (uint32_t)st[14], (uint32_t)st[15]};
}

__device__ __forceinline__ void duel_store(int32_t *st, const DuelRegs &r)
{
    st[0] = r.pending; st[1] = r.bx; st[2] = r.by; st[3] = r.vx; st[4] = r.vy; st[5] = r.p0; st[6] = r.p1;
    st[7] = r.s0; st[8] = r.s1; st[9] = r.cum0; st[10] = r.cum1; st[11] = r.ended;
    st[12] = (int32_t)r.h0; st[13] = (int32_t)r.h1; st[14] = (int32_t)r.h2; st[15] = (int32_t)r.h3;
}

// books action a of agent-step `step` (actor step & 1) as duel_step_kernel books it at t = step + 1 -> what the actor is
// credited with under "next"
__device__ __forceinline__ int duel_book(DuelRegs &r, int step, int a, int n_actions, uint64_t seed, int64_t ordinal,
                                         int points_to_win)
{
    if ((step & 1) == 0) {   // first_0: the action waits for second_0's
        r.pending = a;
        r.cum0 = 0;
        return r.cum1;
    }
    r.p0 = duel_move(r.p0, r.pending, n_actions);
    r.p1 = duel_move(r.p1, a, n_actions);
    const int r0 = duel_world(r.bx, r.by, r.vx, r.vy, r.p0, r.p1, r.s0, r.s1, r.ended, step + 1, seed, ordinal, points_to_win);
    r.h0 = r.h1; r.h1 = r.h2; r.h2 = r.h3; r.h3 = duel_snapshot(r.bx, r.by, r.p0, r.p1);
    r.pending = COEVO_DUEL_NO_ACTION;
    r.cum0 += r0;
    r.cum1 = -r0;
    return r.cum0;
}

// COEVO_DUEL_SEAT_TRACKER for player s on the newest snapshot word
__device__ __forceinline__ int duel_tracker(uint32_t word, int s)
{
    const int bx = word & 255, by = (word >> 8) & 255, p = s ? (int)(word >> 24) : (int)((word >> 16) & 255), X = s ? 78 : 4;
    const bool hidden = bx <= X && X <= bx + 1 && by + 1 >= p && by <= p + 11;   // the ball covers paddle rows in column X
    const int top = hidden ? min(p, by) : p;
    const int d = 2 * by + 2 - (2 * top + 12);
    return (d >= -4 && d <= 4) ? 0 : (d < 0 ? 2 : 3);
}

constexpr int SEAT_NO_OUT = 0, SEAT_OUT_F32 = 1, SEAT_OUT_F16 = 2;
template <int OUT>
__global__ __launch_bounds__(COEVO_DUEL_THREADS) void duel_seat_step_kernel(
    int32_t *gstate, double *acc, int n_games, const int64_t *game_ordinal0, const int32_t *gen_dev, int64_t ordinals_per_gen,
    int t, const int32_t *limit, const int32_t *seats, int script_parity, const int32_t *row_prev, int32_t *actions_prev,
    int32_t *script_actions, const int32_t *row_next, uint8_t *frames, int C, int n_actions, uint64_t seed, int points_to_win,
    int own, const float *slab, const coevo_dqn_task *tasks_prev, int n_tasks_prev, const float *hid, int32_t *status)
{
    const int g = blockIdx.x;
    if (g >= n_games) return;
    const int64_t ordinal = game_ordinal0[g] + (gen_dev ? (int64_t)(*gen_dev) * ordinals_per_gen : 0);
    const int lim = (ordinal < 0) ? 0 : limit[g];   // a negative ordinal disables the game
    int32_t *st = gstate + (size_t)DW * g;
    constexpr bool FUSED = OUT != SEAT_NO_OUT, H16 = OUT == SEAT_OUT_F16;
    __shared__ uint32_t s_snap[4];
    __shared__ int s_render;
    __shared__ __attribute__((aligned(16))) float xs[FUSED ? DQ_FC1_OUT : 4];
    __shared__ float lg[FUSED ? 64 : 1];
    int action = 0;
    bool stale = false;   // the fp16 row of a bad task: nothing is computed, the stored word is booked
    if constexpr (FUSED) {
        // every thread reads `ended` (t >= 1 here).  Thread 0 stores the state only after a booking; the net's needs this very
        // condition and the seat's cannot happen without it (t < lim implies t - 1 < lim), so the store comes behind the
        // barriers of dqn_out_row: no thread can see the new value.  Workgroup-uniform.
        if (t - 1 < lim && st[11] == 0) {
            const int row = row_prev[g];
            const coevo_dqn_task task = tasks_prev[task_of_row(tasks_prev, n_tasks_prev, row)];
            if constexpr (H16) stale = dqn16_bad_task(task);   // before any load through net_off and every barrier
            if (!stale) {
                action = dqn_out_row<H16>(slab + task.net_off, H16 ? dqn16_layout(C, n_actions) : dqn_layout(C, n_actions),
                                          n_actions, hid + (size_t)row * DQ_FC1_OUT, nullptr, status, xs, lg, threadIdx.x);
                if (threadIdx.x == 0) actions_prev[row] = action;
            }
        }
    }
    if (threadIdx.x == 0) {
        DuelRegs r;
        double a_net = 0.0, a_seat = 0.0;   // acc of the net's parity and of the seat's
        double *acc_g = acc + 3 * (size_t)g;
        bool booked_net = false, booked_seat = false;
        if (t == 0) {
            const DuelBall b = duel_serve(seed, ordinal, 0);
            const uint32_t h = duel_snapshot(b.bx, b.by, 36, 36);
            r = {COEVO_DUEL_NO_ACTION, b.bx, b.by, b.vx, b.vy, 36, 36, 0, 0, 0, 0, 0, h, h, h, h};
        } else {
            r = duel_load(st);
            a_seat = acc_g[script_parity];
            if (t - 1 < lim && r.ended == 0) {   // the net's step t-1
                const int a = (FUSED && !stale) ? action : actions_prev[row_prev[g]];
                const int credit = duel_book(r, t - 1, a, n_actions, seed, ordinal, points_to_win);
                a_net = acc_g[1 - script_parity] + (double)(own ? -credit : credit);
                booked_net = true;
            }
        }
        if (t < lim && r.ended == 0) {   // the seat's step t, on the state as it now stands
            const int32_t *seat = seats + (size_t)COEVO_DUEL_SEAT_WORDS * g;
            const int kind = seat[0];
            int a = 0;
            bool ok = true;
            if (kind == COEVO_DUEL_SEAT_TRACKER)
                a = duel_tracker(r.h3, script_parity);
            else
                ok = scripted_action(kind, seat[1], (uint32_t)seat[2], (uint32_t)seat[3], [&] { return (uint64_t)ordinal; },
                                     script_parity, (uint32_t)((t - script_parity) >> 1), n_actions, a);
            if (!ok) { a = 0; atomicOr(status, COEVO_ST_BAD_TASK); }
            script_actions[g] = a;
            const int credit = duel_book(r, t, a, n_actions, seed, ordinal, points_to_win);
            a_seat = a_seat + (double)(own ? -credit : credit);
            booked_seat = true;
        }
        if (t == 0 || booked_net || booked_seat) duel_store(st, r);
        if (t == 0) {
            acc_g[0] = a_seat; acc_g[1] = 0.0; acc_g[2] = 0.0;   // (script_parity == 0 here)
        } else {
            if (booked_net) acc_g[1 - script_parity] = a_net;
            if (booked_seat) acc_g[script_parity] = a_seat;
        }
        s_snap[0] = r.h0; s_snap[1] = r.h1; s_snap[2] = r.h2; s_snap[3] = r.h3;
        s_render = (r.ended == 0 && t + 1 < lim) ? 1 : 0;
    }
    __syncthreads();
    if (!frames || !s_render) return;
    const uint32_t snap[4] = {s_snap[0], s_snap[1], s_snap[2], s_snap[3]};
    duel_render(reinterpret_cast<uint4 *>(frames + (size_t)row_next[g] * DUEL_PIXELS * C), snap, C, (t + 1) & 1);
}

}  // namespace coevo

using namespace coevo;

static bool seat_args_ok(const int32_t *state, const double *acc, int n_games, const int64_t *ordinal0, int t, int t_min,
                         const int32_t *limit, const int32_t *seats, int script_parity, const int32_t *row_prev,
                         const int32_t *actions_prev, const int32_t *script_actions, const int32_t *row_next,
                         const uint8_t *frames, int C, int n_actions, int points_to_win, int flags, const int32_t *status)
{
    if (!duel_args_ok(state, acc, n_games, ordinal0, t, t_min, limit, row_prev, actions_prev, row_next, frames, C, n_actions,
                      points_to_win, flags))
        return false;
    if (!seats || !script_actions || !status) return false;
    return (script_parity == 0 || script_parity == 1) && (t & 1) == script_parity;
}

extern "C" int coevo_duel_seat_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0,
                                    const int32_t *gen_dev, int64_t ordinals_per_gen, int t, const int32_t *limit,
                                    const int32_t *seats, int script_parity, const int32_t *row_prev,
                                    const int32_t *actions_prev, int32_t *script_actions, const int32_t *row_next,
                                    uint8_t *frames, int C, int n_actions, uint64_t seed, int points_to_win, int flags,
                                    int32_t *status, void *stream)
{
    if (!seat_args_ok(duel_state, acc, n_games, game_ordinal0, t, 0, limit, seats, script_parity, row_prev, actions_prev,
                      script_actions, row_next, frames, C, n_actions, points_to_win, flags, status))
        return COEVO_ERR_ARG;
    hipLaunchKernelGGL(duel_seat_step_kernel<SEAT_NO_OUT>, dim3(n_games), dim3(COEVO_DUEL_THREADS), 0, (hipStream_t)stream,
                       duel_state, acc, n_games, game_ordinal0, gen_dev, ordinals_per_gen, t, limit, seats, script_parity,
                       row_prev, const_cast<int32_t *>(actions_prev), script_actions, row_next, frames, C, n_actions, seed,
                       points_to_win, flags & COEVO_DUEL_CREDIT_OWN, nullptr, nullptr, 0, nullptr, status);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn_out_duel_seat_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0,
                                            const int32_t *gen_dev, int64_t ordinals_per_gen, int t, const int32_t *limit,
                                            const int32_t *seats, int script_parity, const int32_t *row_prev,
                                            int32_t *actions_prev, int32_t *script_actions, const int32_t *row_next,
                                            uint8_t *frames, int C, int n_actions, uint64_t seed, int points_to_win, int flags,
                                            const float *slab, const coevo_dqn_task *tasks_prev, int n_tasks_prev,
                                            int n_rows_total, const void *workspace, int32_t *status, void *stream)
{
    if (!seat_args_ok(duel_state, acc, n_games, game_ordinal0, t, 1, limit, seats, script_parity, row_prev, actions_prev,
                      script_actions, row_next, frames, C, n_actions, points_to_win, flags, status))
        return COEVO_ERR_ARG;
    if (!slab || !tasks_prev || n_tasks_prev <= 0 || n_rows_total <= 0 || !workspace) return COEVO_ERR_ARG;
    const float *hid = static_cast<const float *>(workspace) + (size_t)n_rows_total * DQ_FC1_IN;   // (deepqn.hip's layout)
    hipLaunchKernelGGL(duel_seat_step_kernel<SEAT_OUT_F32>, dim3(n_games), dim3(COEVO_DUEL_THREADS), 0, (hipStream_t)stream,
                       duel_state, acc, n_games, game_ordinal0, gen_dev, ordinals_per_gen, t, limit, seats, script_parity,
                       row_prev, actions_prev, script_actions, row_next, frames, C, n_actions, seed, points_to_win,
                       flags & COEVO_DUEL_CREDIT_OWN, slab, tasks_prev, n_tasks_prev, hid, status);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn16_out_duel_seat_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0,
                                              const int32_t *gen_dev, int64_t ordinals_per_gen, int t, const int32_t *limit,
                                              const int32_t *seats, int script_parity, const int32_t *row_prev,
                                              int32_t *actions_prev, int32_t *script_actions, const int32_t *row_next,
                                              uint8_t *frames, int C, int n_actions, uint64_t seed, int points_to_win,
                                              int flags, const void *slab, const coevo_dqn_task *tasks_prev, int n_tasks_prev,
                                              int n_rows_total, const void *workspace, int32_t *status, void *stream)
{
    if (!seat_args_ok(duel_state, acc, n_games, game_ordinal0, t, 1, limit, seats, script_parity, row_prev, actions_prev,
                      script_actions, row_next, frames, C, n_actions, points_to_win, flags, status))
        return COEVO_ERR_ARG;
    if (!slab || !tasks_prev || n_tasks_prev <= 0 || n_rows_total <= 0 || !workspace) return COEVO_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(slab) & 15) return COEVO_ERR_ARG;
    const float *hid = static_cast<const float *>(workspace) + (size_t)n_rows_total * DQ_FC1_IN;   // (dqn16.hip's layout)
    hipLaunchKernelGGL(duel_seat_step_kernel<SEAT_OUT_F16>, dim3(n_games), dim3(COEVO_DUEL_THREADS), 0, (hipStream_t)stream,
                       duel_state, acc, n_games, game_ordinal0, gen_dev, ordinals_per_gen, t, limit, seats, script_parity,
                       row_prev, actions_prev, script_actions, row_next, frames, C, n_actions, seed, points_to_win,
                       flags & COEVO_DUEL_CREDIT_OWN, static_cast<const float *>(slab), tasks_prev, n_tasks_prev, hid, status);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
