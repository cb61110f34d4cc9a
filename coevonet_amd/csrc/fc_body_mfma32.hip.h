// Shared-opponent tasks (a HoF member / ES base net applied to many games): a real GEMM with M = rows, so the
// dense layers run on the matrix cores.  v_mfma_f32_32x32x2_f32 with C-in = bias is bit-for-bit the canonical
// sequential-k fmaf chain (tools/mfma_chain_probe.hip), so this kernel and the VALU kernel above give identical bits.
//
// One workgroup = one net x up to 32 rows (the M of a 32x32 tile); wave w owns output columns
//   fc1: [128w, 128w+128) = 4 tiles, fc2: [64w, 64w+64) = 2 tiles.
// A operand (activations, [row][k]) comes from LDS in an image laid out so that one ds_read_b128 per lane feeds four
// consecutive MFMAs; B operand (weights) is the same 16-byte row piece stream as the VALU kernel (W2q), turned into
// two k-pair operands for each of the wave's two column tiles by two v_permlane32_swap.
// Accumulator layout (32x32): col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
#pragma once
#include "fc_forward_common.hip.h"

namespace coevo {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct FcMfmaSmem {
    union {
        float h1a[64][64][4];  // [k/8][lane = 32*(k&1) + row][(k>>1)&3]: A operands of fc2, 64 KiB
        float h2[32][260];
    };
    float xst[COEVO_OBS_STRIDE][32];  // observations transposed [k][row]: A operands of fc1
    float w3s[NACT][260];
    float red[32][8];
    float logit[32][COEVO_LOGIT_STRIDE];
};

__device__ inline int mfma_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

template <int MODE>
__device__ __forceinline__ void fc_policy_mfma_body(const FcArgs &a, FcMfmaSmem &sm, const coevo_fc_task &task)
{
    // these workgroups are the long pole of a cycle when they share CUs with the streaming kernel's waves: let their
    // (few) waves win issue arbitration; the streaming waves are waiting on HBM most of the time anyway
#ifndef COEVO_HEAVY_PRIO
#define COEVO_HEAVY_PRIO 3
#endif
    __builtin_amdgcn_s_setprio(COEVO_HEAVY_PRIO);
    COEVO_STAMP(0);
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lc = l & 31, lh = l >> 5;
    const int D = task.D, nrows = task.n_rows, row0 = task.row_begin;
    const float *net = a.slab + task.net_off;
    int st = 0;

    // ---- all small parameters and the whole fc1 B operand requested up front (one HBM/L2 round trip) ----------
    constexpr int KP = 5;  // k-pairs of fc1 (D <= 10)
    float w1[KP][4], p_b1[4], p_g1[4], p_be1[4], p_b2[2], p_g2[2], p_be2[2];
    {
        const float *b1p = net + fc_off_b1(D), *b2p = net + fc_off_b2(D);
#pragma unroll
        for (int kp = 0; kp < KP; ++kp)
#pragma unroll
            for (int tl = 0; tl < 4; ++tl)
                w1[kp][tl] = (2 * kp < D) ? net[(size_t)(2 * kp + lh) * H1 + 128 * w + 32 * tl + lc] : 0.0f;
#pragma unroll
        for (int tl = 0; tl < 4; ++tl) {
            const int j = 128 * w + 32 * tl + lc;
            p_b1[tl] = b1p[j]; p_g1[tl] = b1p[H1 + j]; p_be1[tl] = b1p[2 * H1 + j];
        }
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            const int j = 64 * w + 32 * tl + lc;
            p_b2[tl] = b2p[j]; p_g2[tl] = b2p[H2 + j]; p_be2[tl] = b2p[2 * H2 + j];
        }
    }
    const float p_b3 = (t < 32 * NACT) ? net[fc_off_b3(D) + t % NACT] : 0.0f;

    if constexpr (MODE >= MODE_FUSED) {
        if (t < 32) {
            float o[COEVO_OBS_STRIDE];
#pragma unroll
            for (int k = 0; k < COEVO_OBS_STRIDE; ++k) o[k] = 0.0f;
            if (t < nrows) {
                const int row = row0 + t;
                mpe_fused_observe(a.state, a.state_next, a.act_prev, a.game_limit, a.n_games, a.row_game[row],
                                  a.row_slot[row], a.cycle, a.pos_first, o);
#pragma unroll
                for (int k = 0; k < 10; ++k)
                    if (!__builtin_isfinite(o[k])) st |= COEVO_ST_BAD_INPUT;
            }
#pragma unroll
            for (int k = 0; k < COEVO_OBS_STRIDE; ++k) sm.xst[k][t] = o[k];
        }
    } else {
        for (int i = t; i < 32 * COEVO_OBS_STRIDE; i += 256) {
            const int r = i / COEVO_OBS_STRIDE, k = i % COEVO_OBS_STRIDE;
            float v = 0.0f;
            if (r < nrows && k < D) {
                if constexpr (MODE == MODE_STATE) {
                    const int row = row0 + r;
                    v = mpe_obs_element(a.state, a.n_games, a.row_game[row], a.row_slot[row], k);
                } else {
                    v = a.obs[(size_t)(row0 + r) * COEVO_OBS_STRIDE + k];
                }
                if (!__builtin_isfinite(v)) st |= COEVO_ST_BAD_INPUT;
            }
            sm.xst[k][r] = v;
        }
    }
    {
        const float *W3 = net + fc_off_w3(D);
        for (int i = t; i < NACT * H2; i += 256) sm.w3s[i >> 8][i & 255] = W3[i];
    }
    __syncthreads();
    COEVO_STAMP(1);

    // ---- fc1 on the matrix cores: 4 column tiles per wave, D/2 k-pairs ---------------------------------------
    f32x16 c1[4];
    {
#pragma unroll
        for (int tl = 0; tl < 4; ++tl) {
#pragma unroll
            for (int r = 0; r < 16; ++r) c1[tl][r] = p_b1[tl];
        }
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            if (2 * kp < D) {  // wave-uniform
                const float av = sm.xst[2 * kp + lh][lc];
#pragma unroll
                for (int tl = 0; tl < 4; ++tl)
                    c1[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, w1[kp][tl], c1[tl], 0, 0, 0);
            }
        }
    }
    // ---- LayerNorm(512): canonical blocks 2w (tiles 0,1) and 2w+1 (tiles 2,3) --------------------------------
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float s01 = half_tree_sum(c1[0][r]) + half_tree_sum(c1[1][r]);
        const float s23 = half_tree_sum(c1[2][r]) + half_tree_sum(c1[3][r]);
        if (lc == 0) { sm.red[mfma_row(r, l)][2 * w] = s01; sm.red[mfma_row(r, l)][2 * w + 1] = s23; }
    }
    __syncthreads();
    float stat[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float *rr = sm.red[mfma_row(r, l)];
        float tot = rr[0];
#pragma unroll
        for (int b = 1; b < 8; ++b) tot = tot + rr[b];
        stat[r] = tot * (1.0f / H1);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int tl = 0; tl < 4; ++tl) c1[tl][r] = c1[tl][r] - stat[r];
        const float s01 = half_tree_sum(c1[0][r] * c1[0][r]) + half_tree_sum(c1[1][r] * c1[1][r]);
        const float s23 = half_tree_sum(c1[2][r] * c1[2][r]) + half_tree_sum(c1[3][r] * c1[3][r]);
        if (lc == 0) { sm.red[mfma_row(r, l)][2 * w] = s01; sm.red[mfma_row(r, l)][2 * w + 1] = s23; }
    }
    __syncthreads();
    {
        const float *ga = p_g1, *bt = p_be1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma_row(r, l);
            const float *rr = sm.red[row];
            float tot = rr[0];
#pragma unroll
            for (int b = 1; b < 8; ++b) tot = tot + rr[b];
            const float rstd = 1.0f / __builtin_sqrtf(tot * (1.0f / H1) + LN_EPS);
#pragma unroll
            for (int tl = 0; tl < 4; ++tl) {
                const float y = __builtin_fmaf(c1[tl][r] * rstd, ga[tl], bt[tl]);
                if (row < nrows && bad_post_relu(y)) st |= COEVO_ST_BAD_FC1;
                const int k = 128 * w + 32 * tl + lc;  // this activation is input k of fc2
                sm.h1a[k >> 3][32 * (k & 1) + row][(k >> 1) & 3] = relu_keep_nan(y);
            }
        }
    }
    asm volatile("" : "+v"(st));   // this phase's status bits settled here (see fc_policy_mfma16_body)
    __syncthreads();
    COEVO_STAMP(2);

    // ---- fc2 on the matrix cores: 2 column tiles per wave, 256 k-pairs ---------------------------------------
    f32x16 c2[2];
    {
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
#pragma unroll
            for (int r = 0; r < 16; ++r) c2[tl][r] = p_b2[tl];
        }
        const float4 *wp = reinterpret_cast<const float4 *>(net + fc_off_w2(D)) + (size_t)w * 128 * 64 + l;
        // software pipeline over k-octets, two register buffers in ping-pong: the other buffer's 2U weight pieces
        // are in flight while this buffer's U octets feed 8U MFMAs
        constexpr int U = 2;
        float4 bufA[2 * U], bufB[2 * U];
        auto issue = [&](float4 (&buf)[2 * U], int ko) {
#pragma unroll
            for (int u = 0; u < 2 * U; ++u) buf[u] = wp[(size_t)(2 * ko + u) * 64];
        };
        auto consume = [&](const float4 (&buf)[2 * U], int ko) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float4 av = *reinterpret_cast<const float4 *>(&sm.h1a[ko + u][l][0]);
                const float aop[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                for (int q = 0; q < 2; ++q) {  // the two k-quads of this octet
                    const float4 x = buf[2 * u + q];
                    const u32x2 s0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x.x), __float_as_uint(x.y), false, false);
                    const u32x2 s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x.z), __float_as_uint(x.w), false, false);
                    c2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(aop[2 * q], __uint_as_float(s0[0]), c2[0], 0, 0, 0);
                    c2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(aop[2 * q], __uint_as_float(s0[1]), c2[1], 0, 0, 0);
                    c2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(aop[2 * q + 1], __uint_as_float(s1[0]), c2[0], 0, 0, 0);
                    c2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(aop[2 * q + 1], __uint_as_float(s1[1]), c2[1], 0, 0, 0);
                }
            }
        };
        issue(bufA, 0);
        int ko = 0;
        for (; ko < 64 - 2 * U; ko += 2 * U) {
            issue(bufB, ko + U);
            __builtin_amdgcn_sched_barrier(0);
            consume(bufA, ko);
            issue(bufA, ko + 2 * U);
            __builtin_amdgcn_sched_barrier(0);
            consume(bufB, ko + U);
        }
        issue(bufB, ko + U);
        __builtin_amdgcn_sched_barrier(0);
        consume(bufA, ko);
        consume(bufB, ko + U);
    }
    COEVO_STAMP(3);
    // ---- LayerNorm(256): canonical block w = this wave's two tiles -------------------------------------------
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float s = half_tree_sum(c2[0][r]) + half_tree_sum(c2[1][r]);
        if (lc == 0) sm.red[mfma_row(r, l)][w] = s;
    }
    __syncthreads();  // every wave is done with h1a: h2 may overwrite it below
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float *rr = sm.red[mfma_row(r, l)];
        stat[r] = (((rr[0] + rr[1]) + rr[2]) + rr[3]) * (1.0f / H2);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        c2[0][r] = c2[0][r] - stat[r];
        c2[1][r] = c2[1][r] - stat[r];
        const float s = half_tree_sum(c2[0][r] * c2[0][r]) + half_tree_sum(c2[1][r] * c2[1][r]);
        if (lc == 0) sm.red[mfma_row(r, l)][w] = s;
    }
    __syncthreads();
    {
        const float *ga = p_g2, *bt = p_be2;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma_row(r, l);
            const float *rr = sm.red[row];
            const float tot = ((rr[0] + rr[1]) + rr[2]) + rr[3];
            const float rstd = 1.0f / __builtin_sqrtf(tot * (1.0f / H2) + LN_EPS);
#pragma unroll
            for (int tl = 0; tl < 2; ++tl) {
                const float y = __builtin_fmaf(c2[tl][r] * rstd, ga[tl], bt[tl]);
                if (row < nrows && bad_post_relu(y)) st |= COEVO_ST_BAD_FC2;
                sm.h2[row][64 * w + 32 * tl + lc] = relu_keep_nan(y);
            }
        }
    }
    asm volatile("" : "+v"(st));   // this phase's status bits settled here (see fc_policy_mfma16_body)
    __syncthreads();
    COEVO_STAMP(4);

    // ---- output layer (N = 5: not worth a tile), argmax, status - as in the VALU kernel ----------------------
    if (t < 32 * NACT) {
        const int r = t / NACT, o = t % NACT;
        const float y = out_chain<8>(p_b3, &sm.w3s[o][0], &sm.h2[r][0]);
        sm.logit[r][o] = y;
    }
    __syncthreads();
    COEVO_STAMP(5);
    if (t < nrows) {
        const FirstMax fm = first_max_action(sm.logit[t], st);
        const int best = fm.best;
        st = fm.st;
        store_action<MODE>(a, row0 + t, best, sm.logit[t]);
    }
    if (st) atomicOr(a.status, st);
    COEVO_STAMP(6);
}

}  // namespace coevo
