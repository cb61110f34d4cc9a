// One env-cycle of one cohort for float16 nets (args.precision == "float16", reference MPE/fcnetwork.py:13): the fp16 twin of
// the fused policy launch in fc_forward.hip.  Replaces the per-agent-step forward of utils/game_logic_functions.py:152-163
// (and the env.step / env.last between two of them, :179-190) for every row of the cohort at once, reading the fp16 slab of
// fc16_layout.hip.h: 0.51x the weight bytes of the fp32 launch.
//
// One workgroup (4 wavefronts of 64) = one task = one net applied to up to COEVO_FC_MAX_ROWS rows, in passes of 8:
//   rows   lane r of wave 0 derives its game's state of this cycle in registers from the previous cycle's buffer and actions
//          (mpe_fused_observe: the fp32 launches' own env body, fp64), the adversary-seat row publishes it; x = f16(obs)
//   fc1    thread t owns outputs t and t + 256: sequential-k fmaf chains from the bias on converted weights, rounded to fp16
//   LN     the canonical reduce: block b = wave (b & 3), half (b >> 2); output rounded to fp16; ReLU
//   fc2    thread t owns output column t and streams its 64 pieces (16 bytes = 8 k, fp16 -> fp32 with the exact
//          v_cvt_f32_f16), several pieces ahead of their use; every converted weight is the B operand of one
//          v_mfma_f32_4x4x1_16B_f32 per row group of four, C-in = the bias: the sequential-k fp32 fmaf chain, bit for bit
//          (tools/mfma4_chain_probe.hip; the same form as the fp32 streaming body).  No f16 MFMA, no v_dot2: their internal
//          sums are not the sequential order.  fp16 subnormals convert exactly and the matrix pipe does not flush them.
//   out    one lane per (row, action), 256-long chain out of LDS, rounded to fp16; first maximum by a strict '>' scan
// A task's 256 KiB of W2h comes from HBM once; the later passes of a task of more than 8 rows re-read it through L2.
#include "coevo_common.hip.h"
#include "fc16_layout.hip.h"

namespace coevo {

#ifndef COEVO_F16_U
#define COEVO_F16_U 4   // 16-byte pieces per lane and buffer (two buffers in ping-pong: 4 .. 8 pieces in flight per lane)
#endif

struct Fc16CycleArgs {
    const uint32_t *slab;
    const coevo_fc_task *heavy;   // workgroups [0, n_heavy): the tasks of many rows first (they run the longest)
    const coevo_fc_task *light;   // workgroups [n_heavy, n_heavy + n_light)
    int n_heavy, n_light;
    const double *state;          // the PREVIOUS cycle's state buffer
    double *state_next;           // written by each game's adversary-seat row
    const int32_t *row_game;
    const int32_t *row_slot;
    const int32_t *act_prev;      // [n_games][3] actions of the previous cycle, by env slot
    int32_t *act_cur;             // [n_games][3] this cycle's actions
    const int32_t *game_limit;    // may be null
    int n_games, cycle, pos_first;
    int32_t *status;
    unsigned long long *stamps;   // may be null: [COEVO_STAMP_SLOTS][2] = {min workgroup start, max workgroup end}
};

struct Fc16CycleSmem {
    static constexpr int RP = F16_R + 1;   // odd row pitch: conflict-free scatter of h1 into the k-quad image
    union {
        // fc1 activations [k/4][row][k%4]: one ds_read_b128 hands lane l the A operands x[4g + l%4][4q .. 4q+3] of row group g
        float h1q[H1 / 4][RP][4];
        float h2[F16_R][260];     // fc2 activations, row pitch 260 keeps 16-byte alignment, shifts banks by 4
    };
    float xs[COEVO_FC_MAX_ROWS][COEVO_OBS_STRIDE];   // f16(obs) of every row of the task
    float w3s[NACT][260];
    float red[F16_R][8];          // LayerNorm partials per (row, 64-feature block)
    float logit[F16_R][COEVO_LOGIT_STRIDE];
};

typedef float f32x4_acc16 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_piece __attribute__((ext_vector_type(4)));

// A per-individual net is read once per launch by one CU: non-temporal, so that the stream does not evict what is reused.
// A cache-resident net (COEVO_TASK_RESIDENT) and a net whose task makes several passes use plain loads.  Cache policy only.
template <bool NT>
__device__ __forceinline__ u32x4_piece load_piece16(const u32x4_piece *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// fc2 of one pass: acc[g][i] = row 4g + i of this lane's column, entered holding the bias
template <bool NT>
__device__ __forceinline__ void fc16_fc2_stream(const u32x4_piece *wp, const Fc16CycleSmem &sm, f32x4_acc16 (&acc)[F16_R / 4],
                                                int l)
{
    constexpr int U = COEVO_F16_U, NG = F16_R / 4, NP = H1 / 8;
    static_assert(NP % (2 * U) == 0, "the pieces are consumed in pairs of buffers");
    u32x4_piece bufA[U], bufB[U];
    auto issue = [&](u32x4_piece (&buf)[U], int kb) {
#pragma unroll
        for (int u = 0; u < U; ++u) buf[u] = load_piece16<NT>(wp + (size_t)(kb + u) * H2);
    };
    auto consume = [&](const u32x4_piece (&buf)[U], int kb) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            _Float16 hv[8];
            __builtin_memcpy(hv, &buf[u], sizeof(hv));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float4 x[NG];
#pragma unroll
                for (int g = 0; g < NG; ++g)
                    x[g] = *reinterpret_cast<const float4 *>(&sm.h1q[2 * (kb + u) + h][4 * g + (l & 3)][0]);
                const float w0 = (float)hv[4 * h], w1 = (float)hv[4 * h + 1], w2 = (float)hv[4 * h + 2], w3 = (float)hv[4 * h + 3];
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x[g].x, w0, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x[g].y, w1, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x[g].z, w2, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x[g].w, w3, acc[g], 0, 0, 0);
            }
        }
    };
    // two register buffers in ping-pong, the order pinned: while one buffer's pieces feed the matrix pipe the other's loads
    // are in flight
    issue(bufA, 0);
    int kb = 0;
    for (; kb < NP - 2 * U; kb += 2 * U) {
        issue(bufB, kb + U);
        __builtin_amdgcn_sched_barrier(0);
        consume(bufA, kb);
        issue(bufA, kb + 2 * U);
        __builtin_amdgcn_sched_barrier(0);
        consume(bufB, kb + U);
    }
    issue(bufB, kb + U);
    __builtin_amdgcn_sched_barrier(0);
    consume(bufA, kb);
    consume(bufB, kb + U);
}

__global__ __launch_bounds__(256, 3) void fc16_cycle_kernel(Fc16CycleArgs a)
{
    __shared__ __attribute__((aligned(16))) Fc16CycleSmem sm;
    const bool heavy = (int)blockIdx.x < a.n_heavy;   // workgroup-uniform
    const coevo_fc_task task = heavy ? a.heavy[blockIdx.x] : a.light[(int)blockIdx.x - a.n_heavy];
    const int D = task.D, n_rows = task.n_rows;
    // a task this kernel cannot serve is skipped and reported (the W2h pieces are 16-byte loads: net_off must be a multiple of
    // 4 words); uniform over the workgroup, before any barrier
    if ((D != 8 && D != 10) || n_rows < 1 || n_rows > COEVO_FC_MAX_ROWS || (task.net_off & 3) != 0) {
        if (threadIdx.x == 0) atomicOr(a.status, COEVO_ST_BAD_TASK);
        return;
    }
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    if (a.stamps && t == 0)
        atomicMin(&a.stamps[2 * (blockIdx.x % COEVO_STAMP_SLOTS)], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    const uint32_t *net = a.slab + task.net_off;
    const _Float16 *W1 = reinterpret_cast<const _Float16 *>(net + F16_W1);
    const _Float16 *W3 = reinterpret_cast<const _Float16 *>(net + f16_off_w3(D));
    const float *b1p = reinterpret_cast<const float *>(net + f16_off_b1(D));
    const float *b2p = reinterpret_cast<const float *>(net + f16_off_b2(D));
    int st = 0;

    // ---- the small parameters of this thread, requested up front: one round trip instead of one per layer ----------------
    const float p_b1a = b1p[t], p_b1b = b1p[t + 256], p_g1a = b1p[H1 + t], p_g1b = b1p[H1 + t + 256];
    const float p_be1a = b1p[2 * H1 + t], p_be1b = b1p[2 * H1 + t + 256];
    const float p_b2 = b2p[t], p_g2 = b2p[H2 + t], p_be2 = b2p[2 * H2 + t];
    const float p_b3 = (w == 0 && l < F16_R * NACT) ? reinterpret_cast<const float *>(net + f16_off_b3(D))[l % NACT] : 0.0f;

    // ---- every row of the task: advance its game in registers, observe, (owner row) publish; x = f16(obs) ----------------
    if (w == 0 && l < COEVO_FC_MAX_ROWS) {
        float o[COEVO_OBS_STRIDE];
#pragma unroll
        for (int k = 0; k < COEVO_OBS_STRIDE; ++k) o[k] = 0.0f;
        if (l < n_rows) {
            const int row = task.row_begin + l;
            mpe_fused_observe(a.state, a.state_next, a.act_prev, a.game_limit, a.n_games, a.row_game[row], a.row_slot[row],
                              a.cycle, a.pos_first, o);
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                o[k] = f16r(o[k]);
                if (!__builtin_isfinite(o[k])) st |= COEVO_ST_BAD_INPUT;
            }
        }
#pragma unroll
        for (int k = 0; k < COEVO_OBS_STRIDE; ++k) sm.xs[l][k] = o[k];
    }
    for (int i = t; i < NACT * H2; i += 256) sm.w3s[i >> 8][i & 255] = (float)W3[i];
    const u32x4_piece *wp = reinterpret_cast<const u32x4_piece *>(net) + t;   // piece (kb, t) = wp[kb * 256]
    const bool plain = (task.reserved & COEVO_TASK_RESIDENT) != 0 || n_rows > F16_R;   // workgroup-uniform
    __syncthreads();

    for (int rg = 0; rg < n_rows; rg += F16_R) {
        const int nr = min(F16_R, n_rows - rg);
        // ---- fc1: outputs t and t + 256; sequential-k chains from the bias, rounded to fp16 ------------------------------
        // (the 20 weights are fetched per pass: kept across the passes they would cost every task 20 registers)
        float a0[F16_R], a1[F16_R];
        {
            float w1a[10], w1b[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                w1a[k] = (k < D) ? (float)W1[k * H1 + t] : 0.0f;
                w1b[k] = (k < D) ? (float)W1[k * H1 + 256 + t] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < F16_R; ++r) { a0[r] = p_b1a; a1[r] = p_b1b; }
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                if (k < D) {   // workgroup-uniform
#pragma unroll
                    for (int r = 0; r < F16_R; ++r) {
                        const float x = sm.xs[rg + r][k];   // rows past the task's last hold zeros
                        a0[r] = __builtin_fmaf(w1a[k], x, a0[r]);
                        a1[r] = __builtin_fmaf(w1b[k], x, a1[r]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < F16_R; ++r) { a0[r] = f16r(a0[r]); a1[r] = f16r(a1[r]); }
        }
        // ---- LayerNorm(512) + ReLU: block b of the canonical reduce is wave (b & 3), half (b >> 2) -----------------------
#pragma unroll
        for (int r = 0; r < F16_R; ++r) {
            const float s0 = wave_tree_sum(a0[r]), s1 = wave_tree_sum(a1[r]);
            if (l == 0) { sm.red[r][w] = s0; sm.red[r][4 + w] = s1; }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < F16_R; ++r) {
            float tot = sm.red[r][0];
#pragma unroll
            for (int b = 1; b < 8; ++b) tot = tot + sm.red[r][b];
            const float mean = tot * (1.0f / H1);
            a0[r] = a0[r] - mean;
            a1[r] = a1[r] - mean;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < F16_R; ++r) {
            const float s0 = wave_tree_sum(a0[r] * a0[r]), s1 = wave_tree_sum(a1[r] * a1[r]);
            if (l == 0) { sm.red[r][w] = s0; sm.red[r][4 + w] = s1; }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < F16_R; ++r) {
            float tot = sm.red[r][0];
#pragma unroll
            for (int b = 1; b < 8; ++b) tot = tot + sm.red[r][b];
            const float rstd = 1.0f / __builtin_sqrtf(tot * (1.0f / H1) + LN_EPS);
            const float y0 = f16r(__builtin_fmaf(a0[r] * rstd, p_g1a, p_be1a));
            const float y1 = f16r(__builtin_fmaf(a1[r] * rstd, p_g1b, p_be1b));
            if (r < nr && (bad_post_relu16(y0) || bad_post_relu16(y1))) st |= COEVO_ST_BAD_FC1;
            // (the previous pass's readers of h2, which shares this storage, are behind the barriers above)
            sm.h1q[t >> 2][r][t & 3] = relu_keep_nan(y0);
            sm.h1q[(t + 256) >> 2][r][t & 3] = relu_keep_nan(y1);
        }
        __syncthreads();

        // ---- fc2: the lane's column t, 64 pieces of 8 k -------------------------------------------------------------------
        f32x4_acc16 acc[F16_R / 4];
#pragma unroll
        for (int g = 0; g < F16_R / 4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[g][i] = p_b2;
        if (plain) fc16_fc2_stream<false>(wp, sm, acc, l);
        else fc16_fc2_stream<true>(wp, sm, acc, l);
#pragma unroll
        for (int r = 0; r < F16_R; ++r) acc[r >> 2][r & 3] = f16r(acc[r >> 2][r & 3]);

        // ---- LayerNorm(256) + ReLU: canonical block b = wave b ------------------------------------------------------------
#pragma unroll
        for (int r = 0; r < F16_R; ++r) {
            const float s = wave_tree_sum(acc[r >> 2][r & 3]);
            if (l == 0) sm.red[r][w] = s;
        }
        __syncthreads();   // also: every wave is done reading h1q, h2 may overwrite it below
#pragma unroll
        for (int r = 0; r < F16_R; ++r) {
            const float *rr = sm.red[r];
            const float tot = ((rr[0] + rr[1]) + rr[2]) + rr[3];
            acc[r >> 2][r & 3] = acc[r >> 2][r & 3] - tot * (1.0f / H2);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < F16_R; ++r) {
            const float d = acc[r >> 2][r & 3];
            const float s = wave_tree_sum(d * d);
            if (l == 0) sm.red[r][w] = s;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < F16_R; ++r) {
            const float *rr = sm.red[r];
            const float tot = ((rr[0] + rr[1]) + rr[2]) + rr[3];
            const float rstd = 1.0f / __builtin_sqrtf(tot * (1.0f / H2) + LN_EPS);
            const float y = f16r(__builtin_fmaf(acc[r >> 2][r & 3] * rstd, p_g2, p_be2));
            if (r < nr && bad_post_relu16(y)) st |= COEVO_ST_BAD_FC2;
            sm.h2[r][t] = relu_keep_nan(y);
        }
        __syncthreads();

        // ---- output layer: one lane per (row, action), 256-long sequential chain out of LDS, rounded to fp16 -------------
        if (w == 0 && l < F16_R * NACT) {
            const int r = l / NACT, o = l % NACT;
            float y = p_b3;
            const float4 *wr = reinterpret_cast<const float4 *>(&sm.w3s[o][0]);
            const float4 *xr = reinterpret_cast<const float4 *>(&sm.h2[r][0]);
#pragma unroll 8
            for (int k = 0; k < H2 / 4; ++k) {
                const float4 wv = wr[k], xv = xr[k];
                y = __builtin_fmaf(wv.x, xv.x, y);
                y = __builtin_fmaf(wv.y, xv.y, y);
                y = __builtin_fmaf(wv.z, xv.z, y);
                y = __builtin_fmaf(wv.w, xv.w, y);
            }
            sm.logit[r][o] = f16r(y);
        }
        __syncthreads();

        // ---- first-max action (strict '>' scan from -inf) on the fp16 logits, status ------------------------------------
        if (w == 0 && l < nr) {
            int best = -1;
            float cur = -__builtin_inff();
#pragma unroll
            for (int o = 0; o < NACT; ++o) {
                const float v = sm.logit[l][o];
                if (!__builtin_isfinite(v)) st |= COEVO_ST_BAD_OUT;
                if (v > cur) { cur = v; best = o; }
            }
            if (best < 0) { st |= COEVO_ST_NO_ACTION; best = 0; }
            const int row = task.row_begin + rg + l;
            a.act_cur[3 * a.row_game[row] + a.row_slot[row]] = best;   // by (game, slot)
        }
        // (the next pass writes red / h1q / logit only behind its own barriers, which wave 0 reaches after these reads)
    }
    if (st) atomicOr(a.status, st);
    if (a.stamps && t == 0)
        atomicMax(&a.stamps[2 * (blockIdx.x % COEVO_STAMP_SLOTS) + 1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

// one launch for both task tables of a cohort's env-cycle (either may be empty); used by coevo_mpe16_rollout
int launch_fc16_cycle(const void *slab, const coevo_fc_task *heavy, int n_heavy, const coevo_fc_task *light, int n_light,
                      const double *state_prev, double *state_next, int n_games, const int32_t *row_game,
                      const int32_t *row_slot, const int32_t *act_prev, int32_t *act_cur, const int32_t *game_limit, int cycle,
                      int pos_first, int32_t *status, uint64_t *stamps, hipStream_t s)
{
    if (n_heavy + n_light <= 0) return COEVO_OK;
    const Fc16CycleArgs a{static_cast<const uint32_t *>(slab), heavy, light, n_heavy, n_light, state_prev, state_next,
                          row_game, row_slot, act_prev, act_cur, game_limit, n_games, cycle, pos_first, status,
                          reinterpret_cast<unsigned long long *>(stamps)};
    hipLaunchKernelGGL(fc16_cycle_kernel, dim3((unsigned)(n_heavy + n_light)), dim3(256), 0, s, a);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

}  // namespace coevo

extern "C" int coevo_mpe16_policy_cycle(const void *slab16, const coevo_fc_task *tasks, int n_tasks, int max_rows_per_task,
                                        const double *state_prev, double *state_next, int n_games, const int32_t *row_game,
                                        const int32_t *row_slot, const int32_t *act_prev, int32_t *act_cur,
                                        const int32_t *game_limit, int cycle, int pos_first, int32_t *status, uint64_t *stamps,
                                        void *stream)
{
    if (!slab16 || !tasks || !state_prev || !state_next || !row_game || !row_slot || !act_prev || !act_cur || !status)
        return COEVO_ERR_ARG;
    if (n_tasks < 0 || n_games <= 0 || cycle < 0 || state_prev == state_next || act_prev == act_cur) return COEVO_ERR_ARG;
    if (max_rows_per_task < 1 || max_rows_per_task > COEVO_FC_MAX_ROWS) return COEVO_ERR_ARG;
    return coevo::launch_fc16_cycle(slab16, nullptr, 0, tasks, n_tasks, state_prev, state_next, n_games, row_game, row_slot,
                                    act_prev, act_cur, game_limit, cycle, pos_first, status, stamps, (hipStream_t)stream);
}
