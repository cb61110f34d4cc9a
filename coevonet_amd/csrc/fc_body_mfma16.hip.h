// The lean shared-opponent body: up to 16 rows per task on v_mfma_f32_16x16x4_f32 (tools/mfma16_chain_probe.hip: the
// same bits as the fmaf chain), <= 128 registers and < 40 KiB of LDS, so that FOUR workgroups fit a CU and the merged
// cycle launch keeps every streaming workgroup resident next to the shared-opponent ones (the 32-row body, fc_body_mfma32.hip.h, costs
// 256 registers and 73 KiB: two workgroups per CU).  Wave w owns fc1 columns [128w, 128w+128) = 8 tiles and fc2 columns
// [64w, 64w+64) = 4 tiles.  Operands of one MFMA: lane (c = l%16, kk = l/16) supplies A[row c][k = 4q + kk] and
// B[k = 4q + kk][column c]; accumulator register i of lane (c, g = l/16) is row 4g + i, column c of the tile.
#pragma once
#include "fc_forward_common.hip.h"

namespace coevo {

struct FcMfma16Smem {
    union {
        // A operands of fc2: h1a[k][row ^ ((k >> 2) & 3)] - the xor makes both the scatter from the accumulator layout
        // and the gather by (row, kk) conflict-free at a pitch of 16
        float h1a[H1][16];
        float h2[16][260];
    };
    float xst[12][16];  // observations transposed [k][row], zero padded to 12 inputs: A operands of fc1
    float w3s[NACT][260];
    float red[16][8] __attribute__((aligned(16)));   // [row][canonical block]: a row's partials are read as 16-byte pieces
    float logit[16][COEVO_LOGIT_STRIDE];
};
static_assert(sizeof(FcMfma16Smem) <= 40960, "four workgroups per CU");

// ---- the LayerNorm passes of the lean shared-opponent body, written like fc_policy_body_c's for FEW ISSUED INSTRUCTIONS.
// A wave holds NT = 8 (LayerNorm 512) or 4 (LayerNorm 256) 16x16 tiles; accumulator register i of lane (lc, lg) is row
// 4 lg + i, column lc of a tile, so per register i the wave owes NT sixteen-lane row sums in each of its four rows of lanes.
// All 4 NT of them go through packed butterflies of 16 values (register i of tile T is value NT * i + T): afterwards lane lc
// holds the row sum of tile lc % NT, and the canonical tile adds (T0 + T1) + (T2 + T3) are two more butterfly levels (fp32
// addition commutes: both partners get the same bits).  -> s[j], NT / 4 registers: lane lc of s[j] holds the block sum of row
// 4 lg + (16 j + lc) / NT, block (lc % NT) / 4 of this wave's canonical blocks.
template <int NT, bool SQUARE>
__device__ __forceinline__ void mfma16_block_sums(const f32x4_acc (&c)[NT], int l, float (&s)[NT / 4])
{
    static_assert(NT == 4 || NT == 8, "one or two canonical blocks per wave");
#pragma unroll
    for (int j = 0; j < NT / 4; ++j) {
        float v[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const float x = c[(16 * j + m) % NT][(16 * j + m) / NT];
            v[m] = SQUARE ? x * x : x;
        }
        float r = packed_row16_sums<16>(v, l);
        r = r + dpp_move<0xB1>(r);   // T0 + T1 | T2 + T3 (| T4 + T5 | T6 + T7)
        r = r + dpp_move<0x4E>(r);   // (T0 + T1) + (T2 + T3)
        s[j] = r;
    }
}

// the lanes with lc % 4 == 0 post the block sums: red[row][first block of the wave + block in the wave]
template <int NT>
__device__ __forceinline__ void mfma16_post_sums(const float (&s)[NT / 4], float (*red)[8], int w, int lc, int lg)
{
    if ((lc & 3) == 0) {
#pragma unroll
        for (int j = 0; j < NT / 4; ++j) red[4 * lg + (16 * j + lc) / NT][(NT / 4) * w + (lc % NT) / 4] = s[j];
    }
}

// Row statistics once per row and wave: lane (lc, lg) combines the NB block partials of row 4 lg + lc % 4 left to right
// (two or one 16-byte reads); register i of every lane then takes its row's value from lane i of its quad (DPP quad_perm).
template <int NB>
__device__ __forceinline__ float mfma16_row_total(const float (*red)[8], int lc, int lg)
{
    const float *rr = red[4 * lg + (lc & 3)];
    const float4 a = *reinterpret_cast<const float4 *>(rr);
    float tot = ((a.x + a.y) + a.z) + a.w;
    if constexpr (NB == 8) {
        const float4 b = *reinterpret_cast<const float4 *>(rr + 4);
        tot = (((tot + b.x) + b.y) + b.z) + b.w;
    }
    return tot;
}
__device__ __forceinline__ void quad_spread(float v, float (&out)[4])
{
    out[0] = dpp_move<0x00>(v); out[1] = dpp_move<0x55>(v); out[2] = dpp_move<0xAA>(v); out[3] = dpp_move<0xFF>(v);
}

template <int MODE>
__device__ __forceinline__ void fc_policy_mfma16_body(const FcArgs &a, FcMfma16Smem &sm, const coevo_fc_task &task)
{
    typedef unsigned u32x2_s __attribute__((ext_vector_type(2)));
    COEVO_STAMP(0);
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lc = l & 15, lg = l >> 4;
    const int D = task.D, nrows = task.n_rows, row0 = task.row_begin, flags = task.reserved;
    const float *net = a.slab + task.net_off;
    int st = 0;

    // ---- W1t, fc1.bias and the LayerNorm(512) affine - (D + 3) * 512 contiguous floats of the slab - by LDS-DMA into the
    //      region that later holds fc2's A operands (26 KiB of its 32), as the per-individual body stages them: requested
    //      first, so they do not queue behind the streaming workgroups' traffic, and NOT held in registers across the env
    //      step, whose fp64 state is this body's register peak (as 53 live registers they cost 24 bytes of scratch at four
    //      workgroups per CU).  Read into registers after the barrier below; the region is rewritten three barriers later.
    constexpr int KS = 3;  // k-steps of fc1 (D <= 12)
    float *par = &sm.h1a[0][0];
    {
        const int n_pieces = (D + 3) * (H1 / 4);
#pragma unroll
        for (int j = 0; j < 7; ++j)
            if (64 * w + 256 * j < n_pieces)   // wave-uniform
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(net + 4 * (t + 256 * j)),
                                                 (__attribute__((address_space(3))) void *)(par + 4 * (64 * w + 256 * j)),
                                                 16, 0, 0);
    }
    float p_b2[4], p_g2[4], p_be2[4];
    {
        const float *b2p = net + fc_off_b2(D);
#pragma unroll
        for (int T = 0; T < 4; ++T) p_b2[T] = b2p[64 * w + 16 * T + lc];
    }
    const float p_b3 = (t < 16 * NACT) ? net[fc_off_b3(D) + t % NACT] : 0.0f;

    if constexpr (MODE >= MODE_FUSED) {
        if (t < 16) {
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
        for (int i = t; i < 16 * COEVO_OBS_STRIDE; i += 256) {
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
    // the LayerNorm(256) affine is not needed before the end of the fc2 stream: requested after the env step (whose fp64
    // state is the register peak of this body - held across it, these eight values were spilled to scratch), still long
    // before the stream's own loads
    {
        const float *b2p = net + fc_off_b2(D);
#pragma unroll
        for (int T = 0; T < 4; ++T) {
            const int j = 64 * w + 16 * T + lc;
            p_g2[T] = b2p[H2 + j]; p_be2[T] = b2p[2 * H2 + j];
        }
    }
    __syncthreads();   // (waits for the LDS-DMA too: the fence counts it on vmcnt)
    COEVO_STAMP(1);
    // (registers: the bias first, then one k-step's eight B operands at a time, the LayerNorm affine only after the matrix
    // instructions - all 48 parameter values at once next to the 32 accumulators were this body's new register peak)
    const float *b1s = par + (size_t)D * H1;

    // ---- fc1: 8 column tiles per wave, ceil(D/4) k-steps --------------------------------------------------
    f32x4_acc c1[8];
#pragma unroll
    for (int T = 0; T < 8; ++T) {
        const float b = b1s[128 * w + 16 * T + lc];
#pragma unroll
        for (int i = 0; i < 4; ++i) c1[T][i] = b;
    }
#pragma unroll
    for (int q = 0; q < KS; ++q) {
        if (4 * q < D) {  // wave-uniform
            const float av = sm.xst[4 * q + lg][lc];
            float w1[8];
#pragma unroll
            for (int T = 0; T < 8; ++T)  // a padded k contributes fma(0, -0, acc) = acc for every acc, -0 included
                w1[T] = (4 * q + lg < D) ? par[(size_t)(4 * q + lg) * H1 + 128 * w + 16 * T + lc] : -0.0f;
#pragma unroll
            for (int T = 0; T < 8; ++T) c1[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w1[T], c1[T], 0, 0, 0);
        }
    }
    float p_g1[8], p_be1[8];
#pragma unroll
    for (int T = 0; T < 8; ++T) {
        const int j = 128 * w + 16 * T + lc;
        p_g1[T] = b1s[H1 + j]; p_be1[T] = b1s[2 * H1 + j];
    }
    // ---- LayerNorm(512): canonical blocks 2w (tiles 0..3) and 2w+1 (tiles 4..7); inside a block feature 16T' + lc:
    //      four tree levels inside the 16-lane row, then (T0 + T1) + (T2 + T3) ---------------------------------
    float s1[2], stat[4];
    mfma16_block_sums<8, false>(c1, l, s1);
    mfma16_post_sums<8>(s1, sm.red, w, lc, lg);
    __syncthreads();
    quad_spread(mfma16_row_total<8>(sm.red, lc, lg) * (1.0f / H1), stat);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int T = 0; T < 8; ++T) c1[T][i] = c1[T][i] - stat[i];
    }
    mfma16_block_sums<8, true>(c1, l, s1);
    mfma16_post_sums<8>(s1, sm.red, w, lc, lg);
    __syncthreads();
    quad_spread(1.0f / __builtin_sqrtf(mfma16_row_total<8>(sm.red, lc, lg) * (1.0f / H1) + LN_EPS), stat);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 4 * lg + i;
        const float rstd = stat[i];
#pragma unroll
        for (int T = 0; T < 8; ++T) {
            const float y = __builtin_fmaf(c1[T][i] * rstd, p_g1[T], p_be1[T]);
            if (row < nrows && bad_post_relu(y)) st |= COEVO_ST_BAD_FC1;
            const int k = 128 * w + 16 * T + lc;  // this activation is input k of fc2
            sm.h1a[k][row ^ ((k >> 2) & 3)] = relu_keep_nan(y);
        }
    }
    // (the status bits of this phase settled HERE: left alone, the compiler keeps the 32 activations alive to test them at
    // the very end of the body and spills across the fc2 stream to make room)
    asm volatile("" : "+v"(st));
    __syncthreads();
    COEVO_STAMP(2);

    // ---- fc2: 4 column tiles per wave, 128 k-steps; B operands of the four tiles from the lane's own 16-byte piece by
    //      a 4x4 (register x 16-lane row) transpose - or, TILED (COEVO_TASK_TILED: the net has a tile-major twin of W2,
    //      transposed once where the net was written), the piece's four registers as they were loaded --------------
    f32x4_acc c2[4];
#pragma unroll
    for (int T = 0; T < 4; ++T)
#pragma unroll
        for (int i = 0; i < 4; ++i) c2[T][i] = p_b2[T];
    auto fc2 = [&](auto tiled) {
        constexpr bool TILED = decltype(tiled)::value;
        const float *w2 = TILED ? a.slab + (int64_t)(flags >> COEVO_TASK_TWIN_SHIFT) * COEVO_TASK_TWIN_UNIT : net + fc_off_w2(D);
        const float4 *wp = reinterpret_cast<const float4 *>(w2) + (size_t)w * 128 * 64 + l;
        constexpr int U = COEVO_HEAVY16_U;
        float4 bufA[U], bufB[U];
        auto issue = [&](float4 (&buf)[U], int kq) {
#pragma unroll
            for (int u = 0; u < U; ++u) buf[u] = wp[(size_t)(kq + u) * 64];
        };
        auto consume = [&](const float4 (&buf)[U], int kq) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = kq + u;
                const float av = sm.h1a[4 * q + lg][lc ^ (q & 3)];  // A[row lc][k = 4q + lg]
                if constexpr (TILED) {
                    c2[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, buf[u].x, c2[0], 0, 0, 0);
                    c2[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, buf[u].y, c2[1], 0, 0, 0);
                    c2[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, buf[u].z, c2[2], 0, 0, 0);
                    c2[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, buf[u].w, c2[3], 0, 0, 0);
                } else {
                    const u32x2_s s02 = __builtin_amdgcn_permlane32_swap(__float_as_uint(buf[u].x), __float_as_uint(buf[u].z), false, false);
                    const u32x2_s s13 = __builtin_amdgcn_permlane32_swap(__float_as_uint(buf[u].y), __float_as_uint(buf[u].w), false, false);
                    const u32x2_s y01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
                    const u32x2_s y23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
                    c2[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __uint_as_float(y01[0]), c2[0], 0, 0, 0);
                    c2[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __uint_as_float(y01[1]), c2[1], 0, 0, 0);
                    c2[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __uint_as_float(y23[0]), c2[2], 0, 0, 0);
                    c2[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __uint_as_float(y23[1]), c2[3], 0, 0, 0);
                }
            }
        };
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
    };
    if (!(flags & COEVO_TASK_TILED))   // workgroup-uniform
        fc2(std::false_type{});
    else
        fc2(std::true_type{});
    COEVO_STAMP(3);
    // ---- LayerNorm(256): canonical block w = this wave's four tiles --------------------------------------------
    float s2[1];
    mfma16_block_sums<4, false>(c2, l, s2);
    mfma16_post_sums<4>(s2, sm.red, w, lc, lg);
    __syncthreads();  // every wave is done with h1a: h2 may overwrite it below
    quad_spread(mfma16_row_total<4>(sm.red, lc, lg) * (1.0f / H2), stat);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int T = 0; T < 4; ++T) c2[T][i] = c2[T][i] - stat[i];
    }
    mfma16_block_sums<4, true>(c2, l, s2);
    mfma16_post_sums<4>(s2, sm.red, w, lc, lg);
    __syncthreads();
    quad_spread(1.0f / __builtin_sqrtf(mfma16_row_total<4>(sm.red, lc, lg) * (1.0f / H2) + LN_EPS), stat);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 4 * lg + i;
        const float rstd = stat[i];
#pragma unroll
        for (int T = 0; T < 4; ++T) {
            const float y = __builtin_fmaf(c2[T][i] * rstd, p_g2[T], p_be2[T]);
            if (row < nrows && bad_post_relu(y)) st |= COEVO_ST_BAD_FC2;
            sm.h2[row][64 * w + 16 * T + lc] = relu_keep_nan(y);
        }
    }
    asm volatile("" : "+v"(st));
    __syncthreads();
    COEVO_STAMP(4);

    // ---- output layer, argmax, status - as in the other bodies ------------------------------------------------
    if (t < 16 * NACT) {
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
