// One world cycle of one simple_adversary game on the fp64 struct-of-arrays state: the body of coevo_mpe_step (mpe_env.hip),
// of its host twin, and of the gauntlet's game loop (gauntlet.hip).
#pragma once
#include "coevo_common.hip.h"

namespace coevo {

// One world cycle (three agent-steps) of every game.  Agent-step index of slot s in cycle c is t = 3c + s; it
// happens only while t < limit (play_MPE breaks at timesteps >= limit, :197) and c < max_cycles (truncation, :204,
// enforced by the caller never launching more cycles).  Credits (quirk Q1):
//   adversary_0 acting at 3c   receives agent_0's cumulative reward  = good reward of world step c
//   agent_0     acting at 3c+1 receives agent_1's cumulative reward  = good reward of world step c
//   agent_1     acting at 3c+2 triggers world step c+1 and receives the adversary's reward of that step
// action_of(i): the action of env slot i in this cycle.
template <class ActionOf>
__host__ __device__ inline void mpe_step_game_with(double *st, int n, int cycle, const int32_t *game_limit, int pos_first, int g,
                                                   ActionOf action_of)
{
    const size_t N = (size_t)n;
    const int limit = game_limit ? game_limit[g] : 0x7fffffff;
    const int t0 = 3 * cycle;
    if (t0 >= limit) return;
    const double rg_prev = st[18 * N + g];
    st[19 * N + g] = st[19 * N + g] + rg_prev;                      // adversary_0 acted
    if (t0 + 1 < limit) st[20 * N + g] = st[20 * N + g] + rg_prev;  // agent_0 acted
    if (t0 + 2 >= limit) return;                                    // agent_1 did not act: no world step
    double d[3];
    const double gx = st[16 * N + g], gy = st[17 * N + g];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int act = action_of(i);
        double u[2] = {0.0, 0.0};
        if (act == 1) u[0] = -1.0;
        if (act == 2) u[0] = +1.0;
        if (act == 3) u[1] = -1.0;
        if (act == 4) u[1] = +1.0;
        double p[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double f = (((u[c] * 5.0) + 0.0) / 1.0) * 0.1;
            double pos = st[(2 * i + c) * N + g], vel = st[(6 + 2 * i + c) * N + g];
            if (pos_first) pos = pos + vel * 0.1;
            vel = vel * 0.75;
            vel = vel + f;
            if (!pos_first) pos = pos + vel * 0.1;
            st[(2 * i + c) * N + g] = pos;
            st[(6 + 2 * i + c) * N + g] = vel;
            p[c] = pos;
        }
        const double dx = p[0] - gx, dy = p[1] - gy;
        d[i] = sqrt(dx * dx + dy * dy);
    }
    const double r_adv = -d[0];
    const double m = (d[2] < d[1]) ? d[2] : d[1];
    const double r_good = -m + d[0];
    st[21 * N + g] = st[21 * N + g] + r_adv;  // agent_1 acted
    st[18 * N + g] = r_good;
}

// the actions are read through game_rows[g][3] (row index per slot)
__host__ __device__ inline void mpe_step_game(double *st, int n, const int32_t *game_rows, const int32_t *actions,
                                              int cycle, const int32_t *game_limit, int pos_first, int g)
{
    mpe_step_game_with(st, n, cycle, game_limit, pos_first, g, [=](int i) { return actions[game_rows[3 * g + i]]; });
}

}  // namespace coevo
