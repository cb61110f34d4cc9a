// Paddle duel: the env-step launch of a two-player ball game WITH dynamics for the DeepQN engines (include/coevo_duel.h states
// the rules and the contract; coevonet_amd/atari_duel.py is the same in plain Python).  It takes the place of the synthetic env's
// launch (synth_step_kernel, dqn_engine.hip) behind the same hooks and keeps its shape: one 256-thread workgroup per game, the
// output layer of the previous agent-step optionally riding in front (dqn_out_row), one thread booking, all threads writing the
// next frame.  Where the synthetic launch pays a Philox block per 16 frame bytes, this one pays one per serve.
//
// Phases of a workgroup:  (1) [fused forms] output row of the actor of step t-1 -> action;  (2) thread 0 books the action, steps
// the world at odd steps, and publishes the four history snapshots and "render" through LDS;  barrier;  (3) all threads render:
// every byte of the game's frame row exactly once, in 16-byte stores, no clearing pass, no atomics.
#include "dqn_common.hip.h"
#include "dqn16_layout.hip.h"
#include "duel_pieces.hip.h"

namespace coevo {

constexpr int DUEL_NO_OUT = 0, DUEL_OUT_F32 = 1, DUEL_OUT_F16 = 2;
template <int OUT>
__global__ __launch_bounds__(COEVO_DUEL_THREADS) void duel_step_kernel(int32_t *gstate, double *acc, int n_games,
                                                                        const int64_t *game_ordinal0, const int32_t *gen_dev,
                                                                        int64_t ordinals_per_gen, int t, const int32_t *limit,
                                                                        const int32_t *row_prev, int32_t *actions_prev,
                                                                        const int32_t *row_cur, uint8_t *frames, int C,
                                                                        int n_actions, uint64_t seed, int points_to_win, int own,
                                                                        const float *slab, const coevo_dqn_task *tasks_prev,
                                                                        int n_tasks_prev, const float *hid, int32_t *status)
{
    const int g = blockIdx.x;
    if (g >= n_games) return;
    const int64_t ordinal = game_ordinal0[g] + (gen_dev ? (int64_t)(*gen_dev) * ordinals_per_gen : 0);
    const int lim = (ordinal < 0) ? 0 : limit[g];   // a negative ordinal disables the game
    int32_t *st = gstate + (size_t)DW * g;
    constexpr bool FUSED = OUT != DUEL_NO_OUT, H16 = OUT == DUEL_OUT_F16;
    __shared__ uint32_t s_snap[4];
    __shared__ int s_render;
    __shared__ __attribute__((aligned(16))) float xs[FUSED ? DQ_FC1_OUT : 4];
    __shared__ float lg[FUSED ? 64 : 1];
    int action = 0;
    bool stale = false;   // the fp16 row of a bad task: nothing is computed, the stored word is booked
    if constexpr (FUSED) {
        // every thread reads `ended` (t >= 1 here).  Thread 0 rewrites the word only when this condition holds, and then behind
        // the barriers of dqn_out_row: no thread can see the new value.  Workgroup-uniform.
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
        int ended;
        uint32_t h0, h1, h2, h3;
        if (t == 0) {
            const DuelBall b = duel_serve(seed, ordinal, 0);
            h0 = h1 = h2 = h3 = duel_snapshot(b.bx, b.by, 36, 36);
            ended = 0;
            st[0] = COEVO_DUEL_NO_ACTION;
            st[1] = b.bx; st[2] = b.by; st[3] = b.vx; st[4] = b.vy; st[5] = 36; st[6] = 36;
            st[7] = 0; st[8] = 0; st[9] = 0; st[10] = 0; st[11] = 0;
            st[12] = (int32_t)h0; st[13] = (int32_t)h0; st[14] = (int32_t)h0; st[15] = (int32_t)h0;
            acc[3 * (size_t)g] = 0.0; acc[3 * (size_t)g + 1] = 0.0; acc[3 * (size_t)g + 2] = 0.0;
        } else {
            ended = st[11];
            h0 = (uint32_t)st[12]; h1 = (uint32_t)st[13]; h2 = (uint32_t)st[14]; h3 = (uint32_t)st[15];
            if (t - 1 < lim && ended == 0) {   // book the action of step t-1 (actor = (t-1) & 1)
                const int a = (FUSED && !stale) ? action : actions_prev[row_prev[g]];
                int credit;
                if (((t - 1) & 1) == 0) {   // first_0: the action waits for second_0's
                    st[0] = a;
                    st[9] = 0;
                    credit = st[10];
                } else {
                    int bx = st[1], by = st[2], vx = st[3], vy = st[4];
                    const int p0 = duel_move(st[5], st[0], n_actions), p1 = duel_move(st[6], a, n_actions);
                    int s0 = st[7], s1 = st[8];
                    const int r0 = duel_world(bx, by, vx, vy, p0, p1, s0, s1, ended, t, seed, ordinal, points_to_win);
                    h0 = h1; h1 = h2; h2 = h3; h3 = duel_snapshot(bx, by, p0, p1);
                    const int cum0 = st[9] + r0;
                    st[0] = COEVO_DUEL_NO_ACTION;
                    st[1] = bx; st[2] = by; st[3] = vx; st[4] = vy; st[5] = p0; st[6] = p1;
                    st[7] = s0; st[8] = s1; st[9] = cum0; st[10] = -r0; st[11] = ended;
                    st[12] = (int32_t)h0; st[13] = (int32_t)h1; st[14] = (int32_t)h2; st[15] = (int32_t)h3;
                    credit = cum0;
                }
                const size_t slot = 3 * (size_t)g + ((t - 1) & 1);
                acc[slot] = acc[slot] + (double)(own ? -credit : credit);
            }
        }
        s_snap[0] = h0; s_snap[1] = h1; s_snap[2] = h2; s_snap[3] = h3;
        s_render = (ended == 0 && t < lim) ? 1 : 0;
    }
    __syncthreads();
    if (!frames || !s_render) return;
    const uint32_t snap[4] = {s_snap[0], s_snap[1], s_snap[2], s_snap[3]};
    uint4 *dst = reinterpret_cast<uint4 *>(frames + (size_t)row_cur[g] * DUEL_PIXELS * C);
    duel_render(dst, snap, C, t & 1);
}

}  // namespace coevo

using namespace coevo;

extern "C" int coevo_duel_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0,
                               const int32_t *gen_dev, int64_t ordinals_per_gen, int t, const int32_t *limit,
                               const int32_t *row_prev, const int32_t *actions_prev, const int32_t *row_cur, uint8_t *frames,
                               int C, int n_actions, uint64_t seed, int points_to_win, int flags, void *stream)
{
    if (!duel_args_ok(duel_state, acc, n_games, game_ordinal0, t, 0, limit, row_prev, actions_prev, row_cur, frames, C,
                      n_actions, points_to_win, flags))
        return COEVO_ERR_ARG;
    hipLaunchKernelGGL(duel_step_kernel<DUEL_NO_OUT>, dim3(n_games), dim3(COEVO_DUEL_THREADS), 0, (hipStream_t)stream, duel_state,
                       acc, n_games, game_ordinal0, gen_dev, ordinals_per_gen, t, limit, row_prev,
                       const_cast<int32_t *>(actions_prev), row_cur, frames, C, n_actions, seed, points_to_win,
                       flags & COEVO_DUEL_CREDIT_OWN, nullptr, nullptr, 0, nullptr, nullptr);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn_out_duel_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0,
                                       const int32_t *gen_dev, int64_t ordinals_per_gen, int t, const int32_t *limit,
                                       const int32_t *row_prev, int32_t *actions_prev, const int32_t *row_cur, uint8_t *frames,
                                       int C, int n_actions, uint64_t seed, int points_to_win, int flags, const float *slab,
                                       const coevo_dqn_task *tasks_prev, int n_tasks_prev, int n_rows_total,
                                       const void *workspace, int32_t *status, void *stream)
{
    if (!duel_args_ok(duel_state, acc, n_games, game_ordinal0, t, 1, limit, row_prev, actions_prev, row_cur, frames, C,
                      n_actions, points_to_win, flags))
        return COEVO_ERR_ARG;
    if (!slab || !tasks_prev || n_tasks_prev <= 0 || n_rows_total <= 0 || !workspace || !status) return COEVO_ERR_ARG;
    const float *hid = static_cast<const float *>(workspace) + (size_t)n_rows_total * DQ_FC1_IN;   // (deepqn.hip's layout)
    hipLaunchKernelGGL(duel_step_kernel<DUEL_OUT_F32>, dim3(n_games), dim3(COEVO_DUEL_THREADS), 0, (hipStream_t)stream, duel_state,
                       acc, n_games, game_ordinal0, gen_dev, ordinals_per_gen, t, limit, row_prev, actions_prev, row_cur, frames,
                       C, n_actions, seed, points_to_win, flags & COEVO_DUEL_CREDIT_OWN, slab, tasks_prev, n_tasks_prev, hid,
                       status);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn16_out_duel_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0,
                                         const int32_t *gen_dev, int64_t ordinals_per_gen, int t, const int32_t *limit,
                                         const int32_t *row_prev, int32_t *actions_prev, const int32_t *row_cur, uint8_t *frames,
                                         int C, int n_actions, uint64_t seed, int points_to_win, int flags, const void *slab,
                                         const coevo_dqn_task *tasks_prev, int n_tasks_prev, int n_rows_total,
                                         const void *workspace, int32_t *status, void *stream)
{
    if (!duel_args_ok(duel_state, acc, n_games, game_ordinal0, t, 1, limit, row_prev, actions_prev, row_cur, frames, C,
                      n_actions, points_to_win, flags))
        return COEVO_ERR_ARG;
    if (!slab || !tasks_prev || n_tasks_prev <= 0 || n_rows_total <= 0 || !workspace || !status) return COEVO_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(slab) & 15) return COEVO_ERR_ARG;
    const float *hid = static_cast<const float *>(workspace) + (size_t)n_rows_total * DQ_FC1_IN;   // (dqn16.hip's layout)
    hipLaunchKernelGGL(duel_step_kernel<DUEL_OUT_F16>, dim3(n_games), dim3(COEVO_DUEL_THREADS), 0, (hipStream_t)stream, duel_state,
                       acc, n_games, game_ordinal0, gen_dev, ordinals_per_gen, t, limit, row_prev, actions_prev, row_cur, frames,
                       C, n_actions, seed, points_to_win, flags & COEVO_DUEL_CREDIT_OWN, static_cast<const float *>(slab),
                       tasks_prev, n_tasks_prev, hid, status);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
