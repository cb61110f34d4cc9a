// Baseline gauntlet (include/coevo_gauntlet.h): a few dozen simple_adversary games of evolved nets against seats that never
// change, every env-cycle of every game in ONE launch.
//
//   coevo_mpe_gauntlet              one workgroup per game plays all its cycles in a loop: observe, three seats, world cycle
//   coevo_mlp_forward_argmax_wave   the PPO policy net with one wave per row, on its own (tests, tools/bench_gauntlet.py)
//
// A training table wants throughput: one thread per policy-net row, thousands of rows, a launch per phase (baseline.hip,
// fc_forward.hip).  A gauntlet has sixty games whose nets are re-read every cycle and nothing else to do with the idle CUs, so
// it is bound by launch gaps and by one lane's latency.  Here a game's cycles are a loop inside one workgroup - no workgroup
// waits for another, no flag, no grid barrier; every loop is bounded by n_cycles - and
//   * an evolved-net seat is fc_policy_body_c<1, MODE_OBS, FC2_DPP>, the small-launch body with plain loads: the champion's
//     0.56 MB stays in cache for the next cycle and for the other episodes of its match;
//   * a policy-net seat is spread over a wave: lane j owns hidden unit j of both layers (its weight rows in registers), the
//     activations reach the other lanes by v_readlane, lanes 0 .. 4 own the logits.  Each output is still its one sequential
//     fmaf chain over k ascending from the bias - the contract of coevo_baseline.h - so logits, action and status are the bits
//     of baseline.hip's mlp_row; only different outputs run on different lanes: a chain of D + 64 + 64 steps, not 5 056;
//   * the seats of a game that are not evolved nets run side by side, slot s on wave s.
// Its own translation unit: whatever else sits in fc_forward.hip reaches the scheduler of the rollout kernels.
#include "baseline_pieces.hip.h"
#include "fc_body_compact.hip.h"
#include "mpe_step.hip.h"

#include "../../include/coevo_gauntlet.h"

namespace coevo {

static_assert(COEVO_GT_THREADS == 256 && COEVO_GT_WAVE_ROWS == 4, "four waves of 64");

// ---- the policy net on one wave ----------------------------------------------------------------------------------------
// what lane l keeps of a net: row l of fc1 and of fc2, and (lanes 0 .. 4; the others repeat row 4) a row of the head
template <int D>
struct MlpLane {
    float w1[D], b1;
    float4 w2[MLP_H / 4];
    float b2;
    float4 w3[MLP_H / 4];
    float b3;
};

template <int D>
__device__ __forceinline__ void mlp_lane_load(MlpLane<D> &p, const float *net, int l)
{
    const float *W1 = net, *b1 = W1 + MLP_H * D, *W2 = b1 + MLP_H, *b2 = W2 + MLP_H * MLP_H, *W3 = b2 + MLP_H,
                *b3 = W3 + MLP_NACT * MLP_H;
#pragma unroll
    for (int k = 0; k < D; ++k) p.w1[k] = W1[l * D + k];
    p.b1 = b1[l];
    const float4 *r2 = reinterpret_cast<const float4 *>(W2 + l * MLP_H);   // 16-byte aligned: net offsets are multiples of 4 floats
#pragma unroll
    for (int q = 0; q < MLP_H / 4; ++q) p.w2[q] = r2[q];
    p.b2 = b2[l];
    const int c = l < MLP_NACT ? l : MLP_NACT - 1;
    const float4 *r3 = reinterpret_cast<const float4 *>(W3 + c * MLP_H);
#pragma unroll
    for (int q = 0; q < MLP_H / 4; ++q) p.w3[q] = r3[q];
    p.b3 = b3[c];
}

__device__ __forceinline__ float lane_value(float v, int lane)   // lane: a constant after unrolling
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float quad_element(const float4 &q, int i) { return i == 0 ? q.x : i == 1 ? q.y : i == 2 ? q.z : q.w; }

// one row on one wave: x = the observation (the same D addresses in every lane) -> the status bits, the action (in every lane)
// and, in lanes 0 .. 4, the row's logits
template <int D>
__device__ __forceinline__ int mlp_wave_row(const MlpLane<D> &p, const float *x, int l, float &logit, int &action)
{
    int st = 0;
    float xv[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xv[k] = x[k];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < D; ++k) bad |= not_finite(xv[k]);
    if (bad) st |= COEVO_ST_BAD_INPUT;
    float a1 = p.b1;
#pragma unroll
    for (int k = 0; k < D; ++k) a1 = __builtin_fmaf(p.w1[k], xv[k], a1);
    if (__any(not_finite(a1))) st |= COEVO_ST_BAD_FC1;
    const float h1 = relu_plus_zero(a1);
    float a2 = p.b2;
#pragma unroll
    for (int k = 0; k < MLP_H; ++k) a2 = __builtin_fmaf(quad_element(p.w2[k >> 2], k & 3), lane_value(h1, k), a2);
    if (__any(not_finite(a2))) st |= COEVO_ST_BAD_FC2;
    const float h2 = relu_plus_zero(a2);
    float a3 = p.b3;
#pragma unroll
    for (int j = 0; j < MLP_H; ++j) a3 = __builtin_fmaf(quad_element(p.w3[j >> 2], j & 3), lane_value(h2, j), a3);
    if (__any(l < MLP_NACT && not_finite(a3))) st |= COEVO_ST_BAD_OUT;
    float lg[MLP_NACT];
#pragma unroll
    for (int c = 0; c < MLP_NACT; ++c) lg[c] = lane_value(a3, c);
    action = first_max(lg);
    logit = a3;
    return st;
}

// coevo_mlp_forward_argmax's task rules; wave w of the workgroup serves rows first + w, first + w + 4, ...
__global__ __launch_bounds__(COEVO_GT_THREADS) void mlp_wave_kernel(const float *nets, int64_t nets_floats, const int32_t *tasks,
                                                                    const float *obs, int n_rows, int32_t *actions,
                                                                    float *logits, int32_t *status)
{
    const int32_t *t = tasks + (size_t)blockIdx.x * COEVO_MLP_TASK_WORDS;
    const int net_off = t[0], first = t[1], count = t[2], D = t[3];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if ((D != 8 && D != 10) || count < 1 || count > MLP_TILE || first < 0 || first > n_rows - count || net_off < 0 ||
        (net_off & 3) || (int64_t)net_off + mlp_stride(D) > nets_floats) {
        if (threadIdx.x == 0) atomicOr(status, COEVO_ST_BAD_TASK);
        return;
    }
    if (w >= count) return;
    auto serve = [&](auto &p) {
        mlp_lane_load(p, nets + net_off, l);
        for (int r = w; r < count; r += COEVO_GT_WAVE_ROWS) {
            const int i = first + r;
            float logit;
            int action;
            const int st = mlp_wave_row(p, obs + (size_t)i * COEVO_OBS_STRIDE, l, logit, action);
            if (logits && l < MLP_NACT) logits[(size_t)i * COEVO_LOGIT_STRIDE + l] = logit;
            if (l == 0) {
                if (st) atomicOr(status, st);
                actions[i] = st ? 0 : action;
            }
        }
    };
    if (D == 10) {
        MlpLane<10> p;
        serve(p);
    } else {
        MlpLane<8> p;
        serve(p);
    }
}

// ---- the gauntlet --------------------------------------------------------------------------------------------------------
struct GauntletArgs {
    const float *slab;
    int64_t slab_floats;
    const float *mlp_nets;
    int64_t mlp_floats;
    const int32_t *games;
    const int64_t *game_ordinal;
    uint64_t ordinal_add;
    double *state;
    const int32_t *game_limit;
    float *obs;
    int32_t *actions;
    int32_t *status;
    int n_games, cycle_first, n_cycles, pos_first;
};

__device__ __forceinline__ int slot_width(int s) { return s == COEVO_SLOT_ADVERSARY ? 8 : 10; }

// is {kind, arg} a seat of slot s that can be played without leaving the slabs?  (the same answer in every thread)
__device__ __forceinline__ bool seat_ok(const GauntletArgs &a, int s, int kind, int arg)
{
    switch (kind) {
    case COEVO_BL_RANDOM: return true;
    case COEVO_BL_PERIODIC: return arg >= 0;
    case COEVO_BL_CONSTANT: return arg >= 0 && arg < NACT;
    case COEVO_GT_FC: return arg >= 0 && !(arg & 3) && (int64_t)arg + fc_params(slot_width(s)) <= a.slab_floats;
    case COEVO_GT_MLP: return arg >= 0 && !(arg & 3) && (int64_t)arg + mlp_stride(slot_width(s)) <= a.mlp_floats;
    default: return false;
    }
}

template <int D>
__device__ __forceinline__ void mlp_seat(const GauntletArgs &a, int arg, const float *x, int l, int row)
{
    MlpLane<D> p;
    mlp_lane_load(p, a.mlp_nets + arg, l);
    float logit;
    int action;
    const int st = mlp_wave_row(p, x, l, logit, action);
    if (l == 0) {
        if (st) atomicOr(a.status, st);
        a.actions[row] = st ? 0 : action;
    }
}

__global__ __launch_bounds__(COEVO_GT_THREADS) void gauntlet_kernel(GauntletArgs a)
{
    __shared__ FcSmemC<1> sm;
    __shared__ float xs[3][COEVO_OBS_STRIDE];   // the cycle's observations, for the seats that are not evolved nets
    const int g = blockIdx.x, t = threadIdx.x, w = t >> 6, l = t & 63;
    const int32_t *gw = a.games + (size_t)g * COEVO_GT_GAME_WORDS;
    const int kind0 = gw[0], arg0 = gw[1], kind1 = gw[4], arg1 = gw[5], kind2 = gw[8], arg2 = gw[9];
    // (every thread of the workgroup sees the same words: the refusal is uniform, nobody is left at a barrier)
    if (!seat_ok(a, 0, kind0, arg0) || !seat_ok(a, 1, kind1, arg1) || !seat_ok(a, 2, kind2, arg2)) {
        if (t == 0) atomicOr(a.status, COEVO_ST_BAD_TASK);
        return;
    }
    const int n = a.n_games, row0 = 3 * g;
    // wave s < 3 plays slot s when it is no evolved net
    const int my_kind = w == 0 ? kind0 : w == 1 ? kind1 : kind2, my_arg = w == 0 ? arg0 : w == 1 ? arg1 : arg2;
    FcArgs fa = {};
    fa.slab = a.slab;
    fa.obs = a.obs;
    fa.actions = a.actions;
    fa.status = a.status;
    fa.n_games = n;

    for (int c = a.cycle_first; c < a.cycle_first + a.n_cycles; ++c) {
        // ---- 1. the three observations: coevo_mpe_observe's values, element by element -----------------------------------
        if (t < 3 * COEVO_OBS_STRIDE) {
            const int s = t / COEVO_OBS_STRIDE, k = t % COEVO_OBS_STRIDE;
            const float v = k < slot_width(s) ? mpe_obs_element(a.state, n, g, s, k) : 0.0f;
            a.obs[(size_t)(row0 + s) * COEVO_OBS_STRIDE + k] = v;
            xs[s][k] = v;
        }
        __syncthreads();
        // ---- 2. the seats: policy nets and scripted seats side by side, then the evolved nets one after the other -------
        if (w < 3) {
            if (my_kind == COEVO_GT_MLP) {
                if (w == 0) mlp_seat<8>(a, my_arg, xs[0], l, row0);
                else mlp_seat<10>(a, my_arg, xs[w], l, row0 + w);
            } else if (my_kind != COEVO_GT_FC && l == 0) {
                int action;
                if (scripted_action(my_kind, my_arg, (uint32_t)gw[4 * w + 2], (uint32_t)gw[4 * w + 3],
                                    [&] { return (uint64_t)a.game_ordinal[g] + a.ordinal_add; }, w, (uint32_t)c, NACT, action))
                    a.actions[row0 + w] = action;
            }
        }
#pragma nounroll
        for (int s = 0; s < 3; ++s) {
            const int kind = s == 0 ? kind0 : s == 1 ? kind1 : kind2;
            if (kind != COEVO_GT_FC) continue;   // workgroup-uniform
            coevo_fc_task task;
            task.net_off = s == 0 ? arg0 : s == 1 ? arg1 : arg2;
            task.row_begin = row0 + s;
            task.n_rows = 1;
            task.D = slot_width(s);
            task.reserved = 0;
            fc_policy_body_c<1, MODE_OBS, FC2_DPP>(fa, sm, &task, 0, 1);
            // `par` and `tail` share storage and wave 0 is still in the output layer when the others return
            __syncthreads();
        }
        __syncthreads();
        // ---- 3. the world cycle of coevo_mpe_step -----------------------------------------------------------------------
        if (t == 0)
            mpe_step_game_with(a.state, n, c, a.game_limit, a.pos_first, g, [&](int i) { return a.actions[row0 + i]; });
        __syncthreads();
    }
}

}  // namespace coevo

extern "C" int coevo_mpe_gauntlet(const float *slab, int64_t slab_floats, const float *mlp_nets, int64_t mlp_floats,
                                  const int32_t *games, int n_games, const int64_t *game_ordinal, uint64_t ordinal_add,
                                  double *state, const int32_t *game_limit, int cycle_first, int n_cycles, int pos_first,
                                  float *obs_scratch, int32_t *actions, int32_t *status, void *stream)
{
    if (!slab || !coevo::aligned16(slab) || slab_floats < 0 || mlp_floats < 0 || (!mlp_nets && mlp_floats != 0) ||
        !coevo::aligned16(mlp_nets) || !games || !game_ordinal || !state || !game_limit || !obs_scratch || !actions || !status ||
        n_games < 0 || cycle_first < 0 || n_cycles < 0 || (int64_t)cycle_first + n_cycles > INT32_MAX / 3)
        return COEVO_ERR_ARG;
    if (n_games == 0 || n_cycles == 0) return COEVO_OK;
    coevo::GauntletArgs a = {slab,  slab_floats, mlp_nets,    mlp_floats, games,  game_ordinal, ordinal_add, state,
                             game_limit, obs_scratch, actions, status, n_games, cycle_first, n_cycles, pos_first ? 1 : 0};
    hipLaunchKernelGGL(coevo::gauntlet_kernel, dim3(n_games), dim3(COEVO_GT_THREADS), 0, (hipStream_t)stream, a);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_mlp_forward_argmax_wave(const float *nets, int64_t nets_floats, const int32_t *tasks, int n_tasks,
                                             const float *obs, int n_rows, int32_t *actions, float *logits, int32_t *status,
                                             void *stream)
{
    if (!nets || !coevo::aligned16(nets) || nets_floats <= 0 || !tasks || !obs || !actions || !status || n_tasks < 0 ||
        n_rows <= 0)
        return COEVO_ERR_ARG;
    if (n_tasks == 0) return COEVO_OK;
    hipLaunchKernelGGL(coevo::mlp_wave_kernel, dim3(n_tasks), dim3(COEVO_GT_THREADS), 0, (hipStream_t)stream, nets, nets_floats,
                       tasks, obs, n_rows, actions, logits, status);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
