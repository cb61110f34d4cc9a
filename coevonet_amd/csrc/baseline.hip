// Baseline opponents (include/coevo_baseline.h): seats of a cross-play that are not evolved nets.
//
//   coevo_baseline_actions      the scripted seats (random / periodic / constant): one thread per seat, one word written
//   coevo_mlp_forward_argmax    the PPO policy net D -> 64 -> 64 -> 5 over observation rows
//   coevo_mpe_mlp_policy_cycle  the same body behind the observation of a (game, slot) seat
//
// The policy net is 5189 floats.  A workgroup stages it once in LDS (20.3 KiB: several workgroups share a CU's 160 KiB) and
// every thread plays ONE whole row: all lanes of a wavefront read a weight at the same LDS address (a broadcast, no bank
// conflict) and multiply it into their own row's value, so each output is the contract's sequential fmaf chain over k
// ascending with nothing to reorder.  The 64 values of the first hidden layer stay in registers (static indices: both loops
// over them are unrolled); a value of the second hidden layer is folded into the five logit chains as soon as it exists - the
// chains still run over k ascending - so the second layer is never stored.  No matrix cores: they would change the summation
// order for no gain at this size.
#include "baseline_pieces.hip.h"

namespace coevo {

// ---- scripted seats --------------------------------------------------------------------------------------------------
__global__ void baseline_actions_kernel(const int32_t *seats, int n_seats, const int64_t *game_ordinal, uint64_t ordinal_add,
                                        int n_games, uint32_t k, int n_actions, int32_t *actions, int n_rows)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_seats) return;
    const int32_t *s = seats + (size_t)i * COEVO_BL_SEAT_WORDS;
    const int game = s[0], row = s[1], kind = s[2], arg = s[3], slot = s[6];
    if (game < 0 || game >= n_games || row < 0 || row >= n_rows) return;
    int action;
    if (!scripted_action(kind, arg, (uint32_t)s[4], (uint32_t)s[5], [=] { return (uint64_t)game_ordinal[game] + ordinal_add; }, slot, k,
                         n_actions, action))
        return;
    actions[row] = action;
}

// ---- the policy net --------------------------------------------------------------------------------------------------
// one row on one thread: w = the net in LDS (flat order), x = the observation -> the five logits and the status bits
template <int D>
__device__ __forceinline__ int mlp_row(const float *w, const float (&x)[10], float (&logit)[MLP_NACT])
{
    const float *W1 = w, *b1 = W1 + MLP_H * D, *W2 = b1 + MLP_H, *b2 = W2 + MLP_H * MLP_H, *W3 = b2 + MLP_H,
                *b3 = W3 + MLP_NACT * MLP_H;
    int st = 0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < D; ++k) bad |= not_finite(x[k]);
    if (bad) st |= COEVO_ST_BAD_INPUT;
    float h[MLP_H];
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < MLP_H; ++j) {
        float a = b1[j];
#pragma unroll
        for (int k = 0; k < D; ++k) a = __builtin_fmaf(W1[j * D + k], x[k], a);
        track_magnitude(m, a);
        h[j] = relu_plus_zero(a);
        if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // (keeps the weight loads of later outputs out of the registers)
    }
    if (magnitude_not_finite(m)) st |= COEVO_ST_BAD_FC1;
#pragma unroll
    for (int c = 0; c < MLP_NACT; ++c) logit[c] = b3[c];
    m = 0;
#pragma unroll 2
    for (int j = 0; j < MLP_H; ++j) {
        float a = b2[j];
#pragma unroll
        for (int k = 0; k < MLP_H; ++k) {
            a = __builtin_fmaf(W2[j * MLP_H + k], h[k], a);
            if ((k & 15) == 15) __builtin_amdgcn_sched_barrier(0);   // sixteen weights in flight, not the whole row
        }
        track_magnitude(m, a);
        const float r = relu_plus_zero(a);
#pragma unroll
        for (int c = 0; c < MLP_NACT; ++c) logit[c] = __builtin_fmaf(W3[c * MLP_H + j], r, logit[c]);
    }
    if (magnitude_not_finite(m)) st |= COEVO_ST_BAD_FC2;
    bad = false;
#pragma unroll
    for (int c = 0; c < MLP_NACT; ++c) bad |= not_finite(logit[c]);
    if (bad) st |= COEVO_ST_BAD_OUT;
    return st;
}

// SEATS: the rows are seats of simple_adversary games (observe from `state`); else rows of `obs`.  One workgroup per task.
template <bool SEATS>
__global__ __launch_bounds__(COEVO_MLP_ROW_TILE) __attribute__((amdgpu_waves_per_eu(4, 4))) void mlp_policy_kernel(
    const float *nets, int64_t nets_floats, const int32_t *tasks, const float *obs, const int32_t *seats, int n_total,
    const double *state, int n_games, int32_t *actions, int n_rows, float *logits, int32_t *status)
{
    __shared__ float4 w4[MLP_LDS_FLOATS / 4];
    const int32_t *t = tasks + (size_t)blockIdx.x * COEVO_MLP_TASK_WORDS;
    const int net_off = t[0], first = t[1], count = t[2], D = t[3];
    const int tid = threadIdx.x;
    // (every thread of the workgroup sees the same task words: the refusal is uniform, nobody is left at the barrier)
    if ((D != 8 && D != 10) || count < 1 || count > MLP_TILE || first < 0 || first > n_total - count || net_off < 0 ||
        (net_off & 3) || (int64_t)net_off + mlp_stride(D) > nets_floats) {
        if (tid == 0) atomicOr(status, COEVO_ST_BAD_TASK);
        return;
    }
    const float4 *src = reinterpret_cast<const float4 *>(nets + net_off);
    for (int i = tid; i < mlp_stride(D) / 4; i += MLP_TILE) w4[i] = src[i];
    __syncthreads();
    if (tid >= count) return;
    const int i = first + tid;
    float x[10];
    int row = i;
    if (SEATS) {
        const int32_t *s = seats + (size_t)i * COEVO_MLP_SEAT_WORDS;
        const int game = s[0], slot = s[2];
        row = s[1];
        if (game < 0 || game >= n_games || row < 0 || row >= n_rows || slot < 0 || slot > 2 ||
            (slot == COEVO_SLOT_ADVERSARY ? 8 : 10) != D) {
            atomicOr(status, COEVO_ST_BAD_TASK);
            return;
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) x[k] = k < D ? mpe_obs_element(state, n_games, game, slot, k) : 0.0f;
    } else {
        const float *o = obs + (size_t)i * COEVO_OBS_STRIDE;
#pragma unroll
        for (int k = 0; k < 10; ++k) x[k] = k < D ? o[k] : 0.0f;
    }
    const float *w = reinterpret_cast<const float *>(w4);
    float logit[MLP_NACT];
    const int st = (D == 10) ? mlp_row<10>(w, x, logit) : mlp_row<8>(w, x, logit);
    if (logits) {
        float *lo = logits + (size_t)i * COEVO_LOGIT_STRIDE;
#pragma unroll
        for (int c = 0; c < MLP_NACT; ++c) lo[c] = logit[c];
    }
    if (st) atomicOr(status, st);
    actions[row] = st ? 0 : first_max(logit);
}

}  // namespace coevo

extern "C" int coevo_mlp_param_count(int D) { return (D == 8 || D == 10) ? coevo::mlp_params(D) : COEVO_ERR_ARG; }
extern "C" int coevo_mlp_slab_stride(int D) { return (D == 8 || D == 10) ? coevo::mlp_stride(D) : COEVO_ERR_ARG; }

extern "C" int coevo_baseline_actions(const int32_t *seats, int n_seats, const int64_t *game_ordinal, uint64_t ordinal_add,
                                      int n_games, uint32_t k, int n_actions, int32_t *actions, int n_rows, void *stream)
{
    if (!seats || !game_ordinal || !actions || n_seats < 0 || n_games <= 0 || n_rows <= 0 || n_actions < 1 || n_actions > 32)
        return COEVO_ERR_ARG;
    if (n_seats == 0) return COEVO_OK;
    hipLaunchKernelGGL(coevo::baseline_actions_kernel, dim3((n_seats + 127) / 128), dim3(128), 0, (hipStream_t)stream, seats,
                       n_seats, game_ordinal, ordinal_add, n_games, k, n_actions, actions, n_rows);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_mlp_forward_argmax(const float *nets, int64_t nets_floats, const int32_t *tasks, int n_tasks,
                                        const float *obs, int n_rows, int32_t *actions, float *logits, int32_t *status,
                                        void *stream)
{
    if (!nets || !coevo::aligned16(nets) || nets_floats <= 0 || !tasks || !obs || !actions || !status || n_tasks < 0 ||
        n_rows <= 0)
        return COEVO_ERR_ARG;
    if (n_tasks == 0) return COEVO_OK;
    hipLaunchKernelGGL(coevo::mlp_policy_kernel<false>, dim3(n_tasks), dim3(COEVO_MLP_ROW_TILE), 0, (hipStream_t)stream, nets,
                       nets_floats, tasks, obs, (const int32_t *)nullptr, n_rows, (const double *)nullptr, 0, actions, n_rows,
                       logits, status);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_mpe_mlp_policy_cycle(const float *nets, int64_t nets_floats, const int32_t *tasks, int n_tasks,
                                          const int32_t *seats, int n_seats, const double *state, int n_games,
                                          int32_t *actions, int n_rows, float *logits, int32_t *status, void *stream)
{
    if (!nets || !coevo::aligned16(nets) || nets_floats <= 0 || !tasks || !seats || !state || !actions || !status ||
        n_tasks < 0 || n_seats <= 0 || n_games <= 0 || n_rows <= 0)
        return COEVO_ERR_ARG;
    if (n_tasks == 0) return COEVO_OK;
    hipLaunchKernelGGL(coevo::mlp_policy_kernel<true>, dim3(n_tasks), dim3(COEVO_MLP_ROW_TILE), 0, (hipStream_t)stream, nets,
                       nets_floats, tasks, (const float *)nullptr, seats, n_seats, state, n_games, actions, n_rows, logits,
                       status);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
