// One workgroup carries P nets (tasks first .. first+P-1).  P = 1 is the plain kernel.  P = 2 is used by the merged
// cycle launch when one net per workgroup would not fit the CUs in a single round: the entry chains (env step,
// observation) and both LayerNorm(512) of the two nets share their latency, the two 512 KiB weight streams run back to
// back, then both LayerNorm(256) / output layers share theirs.  Results do not depend on P.
#pragma once
#include "fc_forward_common.hip.h"

namespace coevo {

template <int R, int P>
struct FcSmem {
    static constexpr int NG = (R + 3) / 4;   // row groups of four = v_mfma_f32_4x4x1 issues per k
    static constexpr int RP = 4 * NG + 1;    // odd row pitch: conflict-free scatter of h1 into the k-quad image
    union {
        // fc1 activations of ONE net at a time, [k/4][row][k%4]: one ds_read_b128 hands lane l the A operands
        // x[4g + l%4][4q .. 4q+3] of row group g.  Rows >= R of the last group are never written: a tile row only
        // feeds its own output row, and nothing reads those.
        float h1q[128][RP][4];
        float h2[P][R][260];  // fc2 activations, row pitch 260 keeps 16-byte alignment, shifts banks by 4
    };
    float xs0[P][R][COEVO_OBS_STRIDE];
    float w3s[P][NACT][260];
    float red[P][R][8];       // LayerNorm partials per (row, 64-feature block)
    float logit[P][R][COEVO_LOGIT_STRIDE];
};

template <int R, int MODE, int P>
__device__ __forceinline__ void fc_policy_body(const FcArgs &a, FcSmem<R, P> &sm, const coevo_fc_task *tasks, int first,
                                               int n_tasks)
{
#ifdef COEVO_LIGHT_PRIO
    __builtin_amdgcn_s_setprio(COEVO_LIGHT_PRIO);
#endif
    COEVO_STAMP(0);
    static_assert(P >= 1 && P <= 4 && R * NACT <= 64, "one wave per net in the per-row phases");
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    int D[P], nrows[P], row0[P];
    const float *net[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const bool active = first + p < n_tasks;  // a missing net repeats the last one with no rows: nothing is written
        const coevo_fc_task task = tasks[active ? first + p : n_tasks - 1];
        D[p] = task.D; nrows[p] = active ? task.n_rows : 0; row0[p] = task.row_begin;
        net[p] = a.slab + task.net_off;
    }
    int st = 0;

    // ---- every small parameter this thread will need, requested up front: one HBM round trip instead of one
    //      per layer (they would otherwise be loaded at first use, behind a barrier, with nothing else in flight).
    //      (Measured: requesting the row lanes' game state even before these - vmcnt completes in order - and marking
    //      consecutive-game tasks to skip the row table costs registers, spills in the paired kernel: 438 vs 451.)
    constexpr int DMAX = 10;
    float w1a[P][DMAX], w1b[P][DMAX];
    float p_b1a[P], p_b1b[P], p_g1a[P], p_g1b[P], p_be1a[P], p_be1b[P];
    float p_b2[P], p_g2[P], p_be2[P];  // fc2 column of this lane: t
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
            w1a[p][k] = (k < D[p]) ? net[p][(size_t)k * H1 + t] : 0.0f;
            w1b[p][k] = (k < D[p]) ? net[p][(size_t)k * H1 + 256 + t] : 0.0f;
        }
        const float *b1p = net[p] + fc_off_b1(D[p]), *b2p = net[p] + fc_off_b2(D[p]);
        p_b1a[p] = b1p[t]; p_b1b[p] = b1p[t + 256];
        p_g1a[p] = b1p[H1 + t]; p_g1b[p] = b1p[H1 + t + 256];
        p_be1a[p] = b1p[2 * H1 + t]; p_be1b[p] = b1p[2 * H1 + t + 256];
        p_b2[p] = b2p[t]; p_g2[p] = b2p[H2 + t]; p_be2[p] = b2p[2 * H2 + t];
    }
    // per-row phases (env step + observation, output layer, argmax): wave p serves net p, lane = row or (row, action)
    const int pw = (w < P) ? w : 0;  // wave-uniform
    const bool row_wave = w < P;
    const float p_b3 = (row_wave && l < R * NACT) ? net[pw][fc_off_b3(D[pw]) + l % NACT] : 0.0f;

    // ---- stage observations (zero padded) and the output layer -------------------------------------------
    if constexpr (MODE >= MODE_FUSED) {
        if (row_wave && l < R) {  // one lane per row: advance its game in registers, observe, (owner row) publish
            float o[COEVO_OBS_STRIDE];
#pragma unroll
            for (int k = 0; k < COEVO_OBS_STRIDE; ++k) o[k] = 0.0f;
            if (l < nrows[pw]) {
                const int row = row0[pw] + l;
                mpe_fused_observe(a.state, a.state_next, a.act_prev, a.game_limit, a.n_games, a.row_game[row],
                                  a.row_slot[row], a.cycle, a.pos_first, o);
#pragma unroll
                for (int k = 0; k < 10; ++k)
                    if (!__builtin_isfinite(o[k])) st |= COEVO_ST_BAD_INPUT;
            }
#pragma unroll
            for (int k = 0; k < COEVO_OBS_STRIDE; ++k) sm.xs0[pw][l][k] = o[k];
        }
    } else {
#pragma unroll
        for (int p = 0; p < P; ++p) {
            for (int i = t; i < R * COEVO_OBS_STRIDE; i += 256) {
                const int r = i / COEVO_OBS_STRIDE, k = i % COEVO_OBS_STRIDE;
                float v = 0.0f;
                if (r < nrows[p] && k < D[p]) {
                    if constexpr (MODE == MODE_STATE) {
                        const int row = row0[p] + r;
                        v = mpe_obs_element(a.state, a.n_games, a.row_game[row], a.row_slot[row], k);
                    } else {
                        v = a.obs[(size_t)(row0[p] + r) * COEVO_OBS_STRIDE + k];
                    }
                    if (!__builtin_isfinite(v)) st |= COEVO_ST_BAD_INPUT;
                }
                sm.xs0[p][r][k] = v;
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const float *W3 = net[p] + fc_off_w3(D[p]);
        for (int i = t; i < NACT * H2; i += 256) sm.w3s[p][i >> 8][i & 255] = W3[i];
    }
    __syncthreads();
    COEVO_STAMP(1);

    // ---- fc1: outputs j0 = t, j1 = t + 256; sequential-k chains from the bias -----------------------------
    float a0[P][R], a1[P][R];
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int r = 0; r < R; ++r) { a0[p][r] = p_b1a[p]; a1[p][r] = p_b1b[p]; }
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
            if (k < D[p]) {  // wave-uniform
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float x = sm.xs0[p][r][k];
                    a0[p][r] = __builtin_fmaf(w1a[p][k], x, a0[p][r]);
                    a1[p][r] = __builtin_fmaf(w1b[p][k], x, a1[p][r]);
                }
            }
        }
    }
    COEVO_STAMP(8);
    // ---- LayerNorm(512) + ReLU: block b of the canonical reduce is wave (b & 3), half (b >> 2) -------------
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s0 = wave_tree_sum(a0[p][r]), s1 = wave_tree_sum(a1[p][r]);
            if (l == 0) { sm.red[p][r][w] = s0; sm.red[p][r][4 + w] = s1; }
        }
    COEVO_STAMP(9);
    __syncthreads();
    COEVO_STAMP(10);
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float tot = sm.red[p][r][0];
#pragma unroll
            for (int b = 1; b < 8; ++b) tot = tot + sm.red[p][r][b];
            const float mean = tot * (1.0f / H1);
            a0[p][r] = a0[p][r] - mean;
            a1[p][r] = a1[p][r] - mean;
        }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s0 = wave_tree_sum(a0[p][r] * a0[p][r]), s1 = wave_tree_sum(a1[p][r] * a1[p][r]);
            if (l == 0) { sm.red[p][r][w] = s0; sm.red[p][r][4 + w] = s1; }
        }
    __syncthreads();
    // the normalised activations stay in registers (a0 / a1) until their net's turn at the single A-operand image
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float tot = sm.red[p][r][0];
#pragma unroll
            for (int b = 1; b < 8; ++b) tot = tot + sm.red[p][r][b];
            const float var = tot * (1.0f / H1);
            const float rstd = 1.0f / __builtin_sqrtf(var + LN_EPS);
            const float y0 = __builtin_fmaf(a0[p][r] * rstd, p_g1a[p], p_be1a[p]);
            const float y1 = __builtin_fmaf(a1[p][r] * rstd, p_g1b[p], p_be1b[p]);
            if (r < nrows[p] && (bad_post_relu(y0) || bad_post_relu(y1))) st |= COEVO_ST_BAD_FC1;
            a0[p][r] = relu_keep_nan(y0);
            a1[p][r] = relu_keep_nan(y1);
        }
    asm volatile("" : "+v"(st));   // this phase's status bits settled here (see fc_policy_mfma16_body)
    COEVO_STAMP(2);
    COEVO_STAMP(11);

    // ---- fc2 on the matrix cores: lane owns output column 64w + l; its streamed 16-byte piece is W2[64w + l][4q..4q+3],
    //      used as is as the B operand of four v_mfma_f32_4x4x1_16B_f32 per row group ------------------------------
    // (Measured: a single left-over row - R = 5 - as VALU FMAs instead of a second 4-row MFMA group halves these
    // workgroups' matrix-pipe use but its serial fma chain and extra broadcast read cost more: 449 vs 516.)
    constexpr int NG = FcSmem<R, P>::NG;
    f32x4_acc acc[P][NG];  // acc[p][g][i]: row 4g + i of net p, column 64w + l
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (p > 0) __syncthreads();  // every wave is done with the previous net's image
#pragma unroll
        for (int r = 0; r < R; ++r) {
            sm.h1q[t >> 2][r][t & 3] = a0[p][r];
            sm.h1q[(t + 256) >> 2][r][t & 3] = a1[p][r];
        }
        __syncthreads();
        COEVO_STAMP(12);
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[p][g][i] = p_b2[p];
        const float4 *wp = reinterpret_cast<const float4 *>(net[p] + fc_off_w2(D[p])) + (size_t)w * 128 * 64 + l;
        // Two register buffers of U pieces in ping-pong, the order pinned with sched_barrier: while one buffer's U
        // pieces feed the matrix pipe the other buffer's U loads are in flight.  (Left alone, the scheduler interleaves
        // loads and MFMAs pairwise with s_waitcnt vmcnt(1) in between - two loads in flight per lane, 28 us per net.
        // Earlier VALU versions of this loop: C++ double buffers were sunk below their consumers, inline-asm loads
        // spilled; with the activations in SGPRs through a global scratch and s_load a lone workgroup ran 22.7 instead
        // of 27 us but the 16 KiB scalar cache thrashed with several workgroups per CU.)
        constexpr int U = COEVO_LIGHT_U;
        static_assert(128 % (2 * U) == 0, "the k-quads are consumed in pairs of buffers");
        float4 bufA[U], bufB[U];
        auto issue = [&](float4 (&buf)[U], int kq) {
#pragma unroll
            for (int u = 0; u < U; ++u) buf[u] = load_stream16(wp + (size_t)(kq + u) * 64);
        };
        auto consume = [&](const float4 (&buf)[U], int kq) { fc2_mfma4_consume<NG, U>(acc[p], buf, sm.h1q, kq, l); };
        issue(bufA, 0);
        int kq = 0;
        for (; kq < 128 - 2 * U; kq += 2 * U) {
            issue(bufB, kq + U);
            __builtin_amdgcn_sched_barrier(0);
            consume(bufA, kq);
            issue(bufA, kq + 2 * U);
            __builtin_amdgcn_sched_barrier(0);
            consume(bufB, kq + U);
        }
        issue(bufB, kq + U);
        __builtin_amdgcn_sched_barrier(0);
        consume(bufA, kq);
        consume(bufB, kq + U);
    }
    COEVO_STAMP(3);
    // ---- LayerNorm(256) + ReLU: canonical block b = wave b ------------------------------------------------------
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s = wave_tree_sum(acc[p][r >> 2][r & 3]);
            if (l == 0) sm.red[p][r][w] = s;
        }
    __syncthreads();  // also: every wave is done reading h1q, h2 may overwrite it below
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float *rr = sm.red[p][r];
            const float tot = ((rr[0] + rr[1]) + rr[2]) + rr[3];
            acc[p][r >> 2][r & 3] = acc[p][r >> 2][r & 3] - tot * (1.0f / H2);
        }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float d = acc[p][r >> 2][r & 3];
            const float s = wave_tree_sum(d * d);
            if (l == 0) sm.red[p][r][w] = s;
        }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float *rr = sm.red[p][r];
            const float tot = ((rr[0] + rr[1]) + rr[2]) + rr[3];
            const float rstd = 1.0f / __builtin_sqrtf(tot * (1.0f / H2) + LN_EPS);
            const float y = __builtin_fmaf(acc[p][r >> 2][r & 3] * rstd, p_g2[p], p_be2[p]);
            if (r < nrows[p] && bad_post_relu(y)) st |= COEVO_ST_BAD_FC2;
            sm.h2[p][r][t] = relu_keep_nan(y);
        }
    asm volatile("" : "+v"(st));   // this phase's status bits settled here (see fc_policy_mfma16_body)
    __syncthreads();
    COEVO_STAMP(4);

    // ---- output layer: one lane per (row, action), 256-long sequential chain out of LDS --------------------
    if (row_wave && l < R * NACT) {
        const int r = l / NACT, o = l % NACT;
        const float y = out_chain<8>(p_b3, &sm.w3s[pw][o][0], &sm.h2[pw][r][0]);
        sm.logit[pw][r][o] = y;
    }
    __syncthreads();
    COEVO_STAMP(5);

    // ---- first-max action (strict '>' scan from -inf), status --------------------------------------------
    if (row_wave && l < nrows[pw]) {
        const FirstMax fm = first_max_action(sm.logit[pw][l], st);
        const int best = fm.best;
        st = fm.st;
        store_action<MODE>(a, row0[pw] + l, best, sm.logit[pw][l]);
    }
    if (st) atomicOr(a.status, st);
    COEVO_STAMP(6);
}

}  // namespace coevo
