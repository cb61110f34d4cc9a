// What the forward bodies of fc_forward.hip share: the launch arguments and modes, the weight-stream load, the diagnostic
// stamps, and the phases that are written once (see fc_forward.hip's opening comment).
#pragma once
#include "coevo_common.hip.h"

namespace coevo {

#ifndef COEVO_HEAVY16_U
#define COEVO_HEAVY16_U 4  // 16-byte pieces per lane and buffer in the lean shared-opponent body (two buffers)
#endif
#ifndef COEVO_LIGHT_U
#define COEVO_LIGHT_U 8   // 16-byte pieces per lane and buffer (two buffers in ping-pong)
#endif

// A per-individual weight set is read exactly once per launch by exactly one CU: non-temporal loads keep that stream
// (335 MB per env-cycle through 32 MB of L2) from evicting what IS reused - the shared-opponent nets and the kernel's own
// code (MI355X_MICROARCH.md row nt-weights).  With the first, VALU-bound version of this kernel they changed nothing
// (350 vs 349 generations/s); with the current one: 539.5 vs 517 (three alternating runs each).
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_acc __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f32_4x4x1 / v_mfma_f32_16x16x4
__device__ inline float4 load_stream16(const float4 *p)
{
    const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t *>(p));
    return make_float4(v[0], v[1], v[2], v[3]);
}

struct FcArgs {
    const float *slab;
    const coevo_fc_task *tasks;
    const float *obs;          // MODE 0: observations given
    const double *state;       // MODE 1: read from the game state [COEVO_MPE_STATE_DOUBLES][n_games];
                               // MODE 2 (fused env step): the PREVIOUS cycle's state buffer
    const int32_t *row_game;
    const int32_t *row_slot;
    int n_games;
    int32_t *actions;
    float *logits;  // may be null
    int32_t *status;
    unsigned long long *stamps;  // may be null: [COEVO_STAMP_SLOTS][2] = {min workgroup start, max workgroup end}
    // MODE 2 only
    double *state_next;          // the buffer this cycle's state is written to (by each game's owner row)
    const int32_t *act_prev;     // [n_games][3] actions of the previous cycle, by env slot
    int32_t *act_cur;            // [n_games][3] this cycle's actions
    const int32_t *game_limit;
    int cycle, pos_first;
    // merged launch only (fc_cycle_kernel): workgroups [0, n_heavy) run `tasks` on the matrix cores, the rest run
    // `light_tasks[blockIdx.x - n_heavy]` through the streaming path
    const coevo_fc_task *light_tasks;
    int n_heavy, n_light;
};
constexpr int MODE_OBS = 0, MODE_STATE = 1, MODE_FUSED = 2;

// 100 MHz wall clock; the first/last workgroup of a launch bracket its duration (used where HIP events cannot be:
// inside hipGraph replays)
// (workgroups spread over COEVO_STAMP_SLOTS slot pairs so that hundreds of simultaneous atomics do not serialise on
// one address; the host takes the min / max over the slots)
__device__ inline void stamp_begin(unsigned long long *stamps)
{
    if (stamps && threadIdx.x == 0)
        atomicMin(&stamps[2 * (blockIdx.x % COEVO_STAMP_SLOTS)], (unsigned long long)__builtin_amdgcn_s_memrealtime());
}
__device__ inline void stamp_end(unsigned long long *stamps)
{
    if (stamps && threadIdx.x == 0)
        atomicMax(&stamps[2 * (blockIdx.x % COEVO_STAMP_SLOTS) + 1],
                  (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

#ifdef COEVO_PHASE_STAMPS
// diagnostic build only (tools/merged_wg_times.py): per-workgroup shader-clock stamps at the phase boundaries of the
// streaming kernel, written to a buffer nothing else reads
__device__ unsigned long long g_phase_stamps[4096 * 16];
#define COEVO_STAMP(i)                                                                          \
    do {                                                                                        \
        if (threadIdx.x == 0 && blockIdx.x < 4096) {                                            \
            /* 100 MHz constant clock: comparable across XCDs (s_memtime is per XCD) */          \
            g_phase_stamps[blockIdx.x * 16 + (i)] = __builtin_amdgcn_s_memrealtime();            \
        }                                                                                       \
    } while (0)
// per-wave stamps (lane 0 of every wave): where do the waves of a workgroup wait for each other?
__device__ unsigned long long g_wave_stamps[4096 * 4 * 16];
#define COEVO_WSTAMP(i)                                                                                         \
    do {                                                                                                        \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096)                                                       \
            g_wave_stamps[(blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
// shader-clock counter (s_memtime) next to the 100 MHz one: effective clock of a section = d(memtime) / d(memrealtime)
#define COEVO_CSTAMP(i)                                                                                         \
    do {                                                                                                        \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096)                                                       \
            g_wave_stamps[(blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + (i)] = __builtin_amdgcn_s_memtime();     \
    } while (0)
#else
#define COEVO_STAMP(i) do { } while (0)
#define COEVO_WSTAMP(i) do { } while (0)
#define COEVO_CSTAMP(i) do { } while (0)
#endif

// Output layer of one (row, action) lane: the 256-long sequential fmaf chain from the bias, W3 row and h2 row out of LDS.
// UNROLL k-quads of both operands are requested at a time (the chain waits for LDS 64 / UNROLL times).
template <int UNROLL>
__device__ __forceinline__ float out_chain(float y, const float *w3row, const float *h2row)
{
    const float4 *wr = reinterpret_cast<const float4 *>(w3row);
    const float4 *xr = reinterpret_cast<const float4 *>(h2row);
#pragma unroll UNROLL
    for (int k = 0; k < H2 / 4; ++k) {
        const float4 wv = wr[k], xv = xr[k];
        y = __builtin_fmaf(wv.x, xv.x, y);
        y = __builtin_fmaf(wv.y, xv.y, y);
        y = __builtin_fmaf(wv.z, xv.z, y);
        y = __builtin_fmaf(wv.w, xv.w, y);
    }
    return y;
}

// U k-quads of the 4x4x1 fc2: lane's streamed piece buf[u] = W2[64 w + l][4 q .. 4 q + 3] is the B operand of four MFMAs per
// row group, the A operands of a row group are one ds_read_b128 of the k-quad image
template <int NG, int U>
__device__ __forceinline__ void fc2_mfma4_consume(f32x4_acc (&acc)[NG], const float4 (&buf)[U],
                                                  const float (*h1q)[4 * NG + 1][4], int kq, int l)
{
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float4 x[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) x[g] = *reinterpret_cast<const float4 *>(&h1q[kq + u][4 * g + (l & 3)][0]);
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x[g].x, buf[u].x, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x[g].y, buf[u].y, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x[g].z, buf[u].z, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x[g].w, buf[u].w, acc[g], 0, 0, 0);
    }
}

// determine_action: the FIRST maximum of a row's NACT logits (strict '>' scan from -inf).  A non-finite logit raises
// COEVO_ST_BAD_OUT in `st`; no logit above -inf (all NaN / -inf) raises COEVO_ST_NO_ACTION and gives action 0.
struct FirstMax { int best, st; };
__device__ __forceinline__ FirstMax first_max_action(const float *lg, int st)
{
    int best = -1;
    float cur = -__builtin_inff();
#pragma unroll
    for (int o = 0; o < NACT; ++o) {
        const float v = lg[o];
        if (!__builtin_isfinite(v)) st |= COEVO_ST_BAD_OUT;
        if (v > cur) { cur = v; best = o; }
    }
    if (best < 0) { st |= COEVO_ST_NO_ACTION; best = 0; }
    return {best, st};
}

// The action of row `row`: by (game, slot) in a fused cycle, by row otherwise; + the optional copy of its logits
template <int MODE>
__device__ __forceinline__ void store_action(const FcArgs &a, int row, int best, const float *lg)
{
    if constexpr (MODE >= MODE_FUSED) {
        a.act_cur[3 * a.row_game[row] + a.row_slot[row]] = best;  // by (game, slot)
    } else {
        a.actions[row] = best;
    }
    if (a.logits) {
#pragma unroll
        for (int o = 0; o < NACT; ++o) a.logits[(size_t)row * COEVO_LOGIT_STRIDE + o] = lg[o];
    }
}

// ---- the packed LayerNorm of the lean bodies: a wave's N = HB * R block sums (R rows x its HB canonical blocks, value
// HB * r + h) come from ONE packed butterfly into red[wave][]; lane r < R then combines row r's 4 HB partials left to right
// (blocks 0..3 = first halves, 4..7 = second halves) and the result is broadcast with v_readlane.  HB = 2: LayerNorm(512),
// HB = 1: LayerNorm(256).  The barriers between the passes are the caller's.
template <int N>
__device__ __forceinline__ void ln_block_sums(const float (&v)[N], float (*red)[16], int w, int l)
{
    const float s = packed_totals<N>(v, l);
    if (l < N) red[w][l] = s;
}

template <int HB>
__device__ __forceinline__ float ln_row_total(const float (*red)[16], int lr)
{
    float tot = red[0][HB * lr];
#pragma unroll
    for (int b = 1; b < 4 * HB; ++b) tot = tot + red[b & 3][HB * lr + (b >> 2)];
    return tot;
}

// second pass: subtract the row means (from the sums in red), post the block sums of the squared deviations to red2
template <int R, int HB>
__device__ __forceinline__ void ln_center(float (&v)[HB * R], const float (*red)[16], float (*red2)[16], int w, int l, int lr)
{
    const float meanv = ln_row_total<HB>(red, lr) * (1.0f / (HB * 256));
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float m = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(meanv), r));
#pragma unroll
        for (int h = 0; h < HB; ++h) v[HB * r + h] = v[HB * r + h] - m;
    }
    float sq[HB * R];
#pragma unroll
    for (int j = 0; j < HB * R; ++j) sq[j] = v[j] * v[j];
    ln_block_sums<HB * R>(sq, red2, w, l);
}

// third pass of LayerNorm(512): affine + ReLU of this thread's two features of every row, into the row-major image (DPP:
// the vector-ALU fc2 reads h1r) or the k-quad image (the 4x4x1 fc2 reads h1q); returns st, COEVO_ST_BAD_FC1 added
template <int R, bool DPP, class SM>
__device__ __forceinline__ int ln512_relu_store(SM &sm, const float (&v)[2 * R], int lr, int nrows, float p_g1a, float p_g1b,
                                                float p_be1a, float p_be1b, int st)
{
    const int t = threadIdx.x;
    const float rstdv = 1.0f / __builtin_sqrtf(ln_row_total<2>(sm.red2, lr) * (1.0f / H1) + LN_EPS);
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float rstd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rstdv), r));
        const float y0 = __builtin_fmaf(v[2 * r] * rstd, p_g1a, p_be1a);
        const float y1 = __builtin_fmaf(v[2 * r + 1] * rstd, p_g1b, p_be1b);
        if (r < nrows) bad = bad || bad_post_relu(y0) || bad_post_relu(y1);
        if constexpr (DPP) {
            sm.h1r[r][t] = relu_keep_nan(y0);
            sm.h1r[r][t + 256] = relu_keep_nan(y1);
        } else {
            sm.h1q[t >> 2][r][t & 3] = relu_keep_nan(y0);
            sm.h1q[(t + 256) >> 2][r][t & 3] = relu_keep_nan(y1);
        }
    }
    if (bad) st |= COEVO_ST_BAD_FC1;
    return st;
}

// third pass of LayerNorm(256): affine + ReLU of column t of every row into h2; returns st, COEVO_ST_BAD_FC2 added
__device__ __forceinline__ float ln256_rstd(const float (*red2)[16], int lr)
{
    return 1.0f / __builtin_sqrtf(ln_row_total<1>(red2, lr) * (1.0f / H2) + LN_EPS);
}
template <int R>
__device__ __forceinline__ int ln256_relu_store(const float (&u)[R], float rstdv, int nrows, float p_g2, float p_be2,
                                                float (*h2)[260], int st)
{
    const int t = threadIdx.x;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float rstd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rstdv), r));
        const float y = __builtin_fmaf(u[r] * rstd, p_g2, p_be2);
        if (r < nrows) bad = bad || bad_post_relu(y);
        h2[r][t] = relu_keep_nan(y);
    }
    if (bad) st |= COEVO_ST_BAD_FC2;
    return st;
}

}  // namespace coevo
