// The per-individual body of the lean merged cycle kernel, written for FEW ISSUED INSTRUCTIONS.
// In a cycle launch all sixteen waves of a CU run the same phase at the same time and the chip clocks at ~1.5 GHz under
// the weight stream, so everything outside the stream is bound by the SIMDs' issue slots, not by latency or instruction
// fetch (tools/merged_wg_times.py: per-wave stamps + shader-clock stamps): with fc1 as 100 VALU FMAs fed by LDS
// broadcasts and one 6-level butterfly per (row, block) value (fc_policy_body) a workgroup spends ~26 of its 67 us between
// the entry barrier and the stream.  Here
//   * fc1 runs on the matrix pipe like fc2 (v_mfma_f32_4x4x1, rows in groups of four: 40 MFMAs instead of 100 FMAs + 70
//     LDS reads), its weights and the LayerNorm parameters staged by LDS-DMA (no registers held across the env step);
//   * the 2 R block sums a wave owes per LayerNorm pass come from ONE packed butterfly (coevo_common.hip.h:
//     packed_totals, ~4 instructions per value instead of 11);
//   * mean / variance / rstd of a row are computed by one lane per row and broadcast with v_readlane, not by every thread;
//   * the stream loop carries its own tail (no peeled copy of the last iteration), the last barrier is a wave fence.
// The arithmetic - every fmaf chain, every reduction tree, the left-to-right block sums - is the canonical one, so the
// bits are those of fc_policy_body and of the oracle.
#pragma once
#include "fc_forward_common.hip.h"

namespace coevo {

template <int R>
struct FcSmemC {
    static constexpr int NG = (R + 3) / 4;   // row groups of four = v_mfma_f32_4x4x1 issues per k
    static constexpr int RP = 4 * NG + 1;    // odd row pitch of the k-quad image (see FcSmem)
    union {
        float par[13 * H1];                  // W1t [D][512], fc1.bias, ln1.weight, ln1.bias: contiguous in the slab
        float h1q[128][RP][4];               // A operands of fc2 (written once every wave is done with `par`)
        float h1r[R][H1];                    // ... row-major for the vector-ALU fc2 of the small-launch kernel (FC2_DPP)
        struct { float h2[R][260]; float w3s[NACT][260]; } tail;   // after the stream
    };
    float xs0[4 * NG][COEVO_OBS_STRIDE];     // observations, rows padded to whole groups (zeros)
    float red[4][16], red2[4][16];           // per wave: its block sums of every row (sums, squared deviations)
    float logit[R][COEVO_LOGIT_STRIDE];
};

// fc2 of the per-individual body, two forms with the same bits (each output is the sequential-k fmaf chain from its bias):
//   FC2_MFMA  v_mfma_f32_4x4x1, rows in groups of four.  The form of the full launch, where several workgroups share a SIMD: a
//             dependent 4x4x1 issues only every 40-56 cycles (tools/mfma_rate_probe.hip chain: one accumulator 40, two 2 x 28),
//             which other workgroups' waves fill.
//   FC2_DPP   v_fmac_f32 with the activation as a DPP row_newbcast source: one VGPR holds 16 consecutive activations of a row
//             (lane % 16 = k), `row_newbcast:j` hands lane j's value to every lane of its 16-lane row inside the fmac - no
//             matrix instruction, no LDS read per k, R independent chains per lane.  The form of a SMALL launch (a rank of a
//             sharded population: fewer workgroups than CUs), where a workgroup has its SIMDs to itself and the two 4x4x1
//             chains of a wave leave the matrix pipe idle 70 % of the time: 512 k x 56 cycles = 12.1 us of a 19 us workgroup
//             (tools/merged_wg_times.py, COEVO_PROBE_SHARD=8), against 512 x R x 6.3 cycles = 6.8 us (tools/fmac_dpp_probe.hip).
//             Its weight stream uses PLAIN loads: a small launch's nets (<= 256 x 0.56 MB) are re-read every env-cycle out of
//             the 256 MiB Infinity Cache, whose shorter latency is bandwidth to a wave with ~16 loads in flight (a rank of 8:
//             16.4 against 18.7 us per launch with nt loads; the full population, 336 MB, streams from HBM and wants nt).
constexpr int FC2_MFMA = 0, FC2_DPP = 1;

#ifndef COEVO_SMALL_U
#define COEVO_SMALL_U 16   // 16-byte pieces per lane and buffer in the small-launch body (two buffers; <= 256 registers)
#endif

template <int J>
__device__ __forceinline__ void fmac_bcast(float &acc, float xv, float w)
{
    // acc = fmaf(xv[lane j of this lane's 16-lane row], w, acc): one rounding, like __builtin_fmaf
    asm("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(xv), "v"(w), "n"(J));
}

// four k-quads (16 consecutive k) of every row's chain: xv[r] holds activations k0 .. k0 + 15 of row r (lane % 16 = k - k0)
template <int R>
__device__ __forceinline__ void fmac_block16(float (&acc)[R], const float (&xv)[R], const float4 &p0, const float4 &p1,
                                             const float4 &p2, const float4 &p3)
{
#define COEVO_FMAC_K(J, W)                                   \
    _Pragma("unroll") for (int r = 0; r < R; ++r) fmac_bcast<J>(acc[r], xv[r], W);
    COEVO_FMAC_K(0, p0.x) COEVO_FMAC_K(1, p0.y) COEVO_FMAC_K(2, p0.z) COEVO_FMAC_K(3, p0.w)
    COEVO_FMAC_K(4, p1.x) COEVO_FMAC_K(5, p1.y) COEVO_FMAC_K(6, p1.z) COEVO_FMAC_K(7, p1.w)
    COEVO_FMAC_K(8, p2.x) COEVO_FMAC_K(9, p2.y) COEVO_FMAC_K(10, p2.z) COEVO_FMAC_K(11, p2.w)
    COEVO_FMAC_K(12, p3.x) COEVO_FMAC_K(13, p3.y) COEVO_FMAC_K(14, p3.z) COEVO_FMAC_K(15, p3.w)
#undef COEVO_FMAC_K
}

// RES (FC2_MFMA only): the task's net is one of the population's cache-resident nets (COEVO_TASK_RESIDENT): its W2 stream
// uses plain loads, which keep the lines in the Infinity Cache for the next env-cycle's read; every other net streams with nt
// loads, which do not evict them (profiles/r06_mall_residency.md).  A template argument, dispatched once per workgroup: the
// cache policy is an immediate of the load instruction.
template <int R, int MODE, int FC2 = FC2_MFMA, bool RES = false>
__device__ __forceinline__ void fc_policy_body_c(const FcArgs &a, FcSmemC<R> &sm, const coevo_fc_task *tasks, int first,
                                                 int n_tasks)
{
    static_assert(!RES || FC2 == FC2_MFMA, "the vector-ALU form streams with plain loads already");
    static_assert((MODE == MODE_FUSED || MODE == MODE_OBS) && R * NACT <= 64 && R <= 8, "the lean merged cycle kernel");
    constexpr int NG = FcSmemC<R>::NG;
    COEVO_STAMP(0);
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const bool active = first < n_tasks;
    const coevo_fc_task task = tasks[active ? first : n_tasks - 1];
    const int D = task.D, nrows = active ? task.n_rows : 0, row0 = task.row_begin;
    const float *net = a.slab + task.net_off;
    int st = 0;

    // ---- W1t, fc1.bias and the LayerNorm(512) affine: (D + 3) * 512 contiguous floats, by LDS-DMA in 16-byte pieces (a
    //      wave's 64 pieces land contiguously at its wave-uniform base; (D + 3) * 128 pieces are a multiple of 64) ------
    const int n_pieces = (D + 3) * (H1 / 4);
#pragma unroll
    for (int j = 0; j < 7; ++j)
        if (64 * w + 256 * j < n_pieces)   // wave-uniform
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(net + 4 * (t + 256 * j)),
                                             (__attribute__((address_space(3))) void *)(&sm.par[4 * (64 * w + 256 * j)]),
                                             16, 0, 0);
    const float *b2p = net + fc_off_b2(D);
    float w3r[5];
    {
        const float *W3 = net + fc_off_w3(D);
#pragma unroll
        for (int j = 0; j < 5; ++j) w3r[j] = W3[t + 256 * j];
    }
    const float p_b2 = b2p[t], p_g2 = b2p[H2 + t], p_be2 = b2p[2 * H2 + t];
    const float p_b3 = (w == 0 && l < R * NACT) ? net[fc_off_b3(D) + l % NACT] : 0.0f;
    constexpr int US = COEVO_SMALL_U;
    static_assert(US % 4 == 0 && 128 % (2 * US) == 0, "buffers of whole 16-k blocks, consumed in pairs");
    const float4 *wps = reinterpret_cast<const float4 *>(net + fc_off_w2(D)) + (size_t)w * 128 * 64 + l;
    float4 sbufA[FC2 == FC2_DPP ? US : 1], sbufB[FC2 == FC2_DPP ? US : 1];

    // ---- env step + observation: one lane per row (wave 0) ----------------------------------------------------
    if (w == 0 && l < 4 * NG) {
        float o[COEVO_OBS_STRIDE];
#pragma unroll
        for (int k = 0; k < COEVO_OBS_STRIDE; ++k) o[k] = 0.0f;
        if (l < nrows) {
            const int row = row0 + l;
            if constexpr (MODE == MODE_FUSED) {
                mpe_fused_observe(a.state, a.state_next, a.act_prev, a.game_limit, a.n_games, a.row_game[row],
                                  a.row_slot[row], a.cycle, a.pos_first, o);
            } else {   // observations given (env stepped elsewhere, e.g. on the host cores): columns >= D are not inputs
#pragma unroll
                for (int k = 0; k < 10; ++k) o[k] = (k < D) ? a.obs[(size_t)row * COEVO_OBS_STRIDE + k] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 10; ++k)
                if (!__builtin_isfinite(o[k])) st |= COEVO_ST_BAD_INPUT;
        }
#pragma unroll
        for (int k = 0; k < COEVO_OBS_STRIDE; ++k) sm.xs0[l][k] = o[k];   // rows R .. 4 NG - 1: zeros (tile padding)
    }
    COEVO_WSTAMP(0);
    __syncthreads();   // (waits for the LDS-DMA too: the fence counts it on vmcnt)
    COEVO_WSTAMP(1);
    COEVO_CSTAMP(10);
    COEVO_STAMP(1);
    // FC2_DPP: the first two buffers of the fc2 stream (a quarter of the net at U = 16) are requested NOW - fc1 and
    // LayerNorm(512) take ~2 us in which nothing else is in flight; the barriers below do not drain them.  (Requested before
    // the entry barrier they delayed it by 1.7 us: that barrier's vmcnt(0) covers the LDS-DMA and, in order, everything else,
    // and wave 0's game-state reads queued behind 32 KiB of stream.)
    if constexpr (FC2 == FC2_DPP) {
#pragma unroll
        for (int uu = 0; uu < US; ++uu) sbufA[uu] = wps[(size_t)uu * 64];
#pragma unroll
        for (int uu = 0; uu < US; ++uu) sbufB[uu] = wps[(size_t)(US + uu) * 64];
    }

    // ---- fc1 on the matrix cores, like fc2: wave w owns features 64 w + l (block w) and 256 + 64 w + l (block 4 + w);
    //      sequential-k chains from the bias, one k per v_mfma_f32_4x4x1 (rows in groups of four) ---------------------
    const float *b1s = sm.par + D * H1;
    f32x4_acc c0[NG], c1[NG];
    {
        const float bia = b1s[t], bib = b1s[t + 256];
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) { c0[g][i] = bia; c1[g][i] = bib; }
        float4 xk[NG][3];   // observations of row 4 g + l % 4: 12 floats (10 used)
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int j = 0; j < 3; ++j) xk[g][j] = *reinterpret_cast<const float4 *>(&sm.xs0[4 * g + (l & 3)][4 * j]);
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            if (k < D) {   // wave-uniform
                const float wa = sm.par[k * H1 + t], wb = sm.par[k * H1 + 256 + t];
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const float4 xv = xk[g][k >> 2];
                    const float x = (k & 3) == 0 ? xv.x : (k & 3) == 1 ? xv.y : (k & 3) == 2 ? xv.z : xv.w;
                    c0[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x, wa, c0[g], 0, 0, 0);
                    c1[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(x, wb, c1[g], 0, 0, 0);
                }
            }
        }
    }
    // LayerNorm parameters of this thread's two features: read before `par` may be overwritten
    const float p_g1a = b1s[H1 + t], p_g1b = b1s[H1 + t + 256], p_be1a = b1s[2 * H1 + t], p_be1b = b1s[2 * H1 + t + 256];
    COEVO_STAMP(8);
    // ---- LayerNorm(512) + ReLU.  Per wave 2 R block sums (rows x its two blocks): one packed butterfly; the eight
    //      partials of a row are combined and turned into mean / rstd by ONE lane per row, then broadcast ---------------
    float v[2 * R];
#pragma unroll
    for (int r = 0; r < R; ++r) { v[2 * r] = c0[r >> 2][r & 3]; v[2 * r + 1] = c1[r >> 2][r & 3]; }
    ln_block_sums<2 * R>(v, sm.red, w, l);          // red[wave][2 r + half]: block (4 half + wave) of row r
    COEVO_STAMP(9);
    COEVO_WSTAMP(2);
    __syncthreads();
    COEVO_WSTAMP(3);
    COEVO_STAMP(10);
    const int lr = l < R ? l : R - 1;             // lane r < R works on row r (the other lanes repeat the last row)
    ln_center<R, 2>(v, sm.red, sm.red2, w, l, lr);
    COEVO_WSTAMP(4);
    __syncthreads();   // every wave is also done with `par` (its fc1 weights and LayerNorm parameters are in registers)
    COEVO_WSTAMP(5);
    st = ln512_relu_store<R, FC2 == FC2_DPP>(sm, v, lr, nrows, p_g1a, p_g1b, p_be1a, p_be1b, st);
    COEVO_WSTAMP(6);
    __syncthreads();
    COEVO_WSTAMP(7);
    COEVO_CSTAMP(11);
    COEVO_STAMP(2);

    // ---- fc2 on the matrix cores, as in fc_policy_body; the ping-pong loop carries its own tail ------------------
    f32x4_acc acc[NG];
    float u[R];
    if constexpr (FC2 == FC2_MFMA) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[g][i] = p_b2;
    {
        const float4 *wp = reinterpret_cast<const float4 *>(net + fc_off_w2(D)) + (size_t)w * 128 * 64 + l;
        constexpr int U = COEVO_LIGHT_U;
        static_assert(128 % (2 * U) == 0, "the k-quads are consumed in pairs of buffers");
        float4 bufA[U], bufB[U];
        auto issue = [&](float4 (&buf)[U], int kq) {
#pragma unroll
            for (int u = 0; u < U; ++u) buf[u] = RES ? wp[(size_t)(kq + u) * 64] : load_stream16(wp + (size_t)(kq + u) * 64);
        };
        auto consume = [&](const float4 (&buf)[U], int kq) { fc2_mfma4_consume<NG, U>(acc, buf, sm.h1q, kq, l); };
        issue(bufA, 0);
#pragma nounroll
        for (int kq = 0; kq < 128; kq += 2 * U) {
            issue(bufB, kq + U);
            __builtin_amdgcn_sched_barrier(0);
            consume(bufA, kq);
            if (kq + 2 * U < 128) issue(bufA, kq + 2 * U);   // wave-uniform
            __builtin_amdgcn_sched_barrier(0);
            consume(bufB, kq + U);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) u[r] = acc[r >> 2][r & 3];
    } else {
        // ---- fc2 on the vector ALU (FC2_DPP, see above): lane = output column 64 w + l, R chains per lane; per 16 k one
        //      ds_read_b32 per row (16 consecutive activations, the same in all four 16-lane rows) and 16 R fmacs ----------
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = p_b2;
        const float *xrow = &sm.h1r[0][l & 15];
        auto issue_s = [&](float4 (&buf)[FC2 == FC2_DPP ? US : 1], int kq) {
#pragma unroll
            for (int uu = 0; uu < US; ++uu) buf[uu] = wps[(size_t)(kq + uu) * 64];   // plain, not nt: see FC2_DPP
        };
        auto consume_s = [&](const float4 (&buf)[FC2 == FC2_DPP ? US : 1], int kq) {
#pragma unroll
            for (int b = 0; b < US / 4; ++b) {
                float xv[R];
#pragma unroll
                for (int r = 0; r < R; ++r) xv[r] = xrow[r * H1 + 4 * (kq + 4 * b)];
                fmac_block16<R>(u, xv, buf[4 * b], buf[4 * b + 1], buf[4 * b + 2], buf[4 * b + 3]);
            }
        };
#pragma nounroll
        for (int kq = 0; kq < 128; kq += 2 * US) {
            consume_s(sbufA, kq);
            if (kq + 2 * US < 128) issue_s(sbufA, kq + 2 * US);   // wave-uniform
            __builtin_amdgcn_sched_barrier(0);
            consume_s(sbufB, kq + US);
            if (kq + 3 * US < 128) issue_s(sbufB, kq + 3 * US);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    COEVO_STAMP(3);
    COEVO_WSTAMP(8);
    COEVO_CSTAMP(12);
    // ---- LayerNorm(256) + ReLU: canonical block b = wave b; R block sums per wave by one packed butterfly ---------------
    ln_block_sums<R>(u, sm.red, w, l);   // (red / red2 live outside the union: no wave still needs the old contents)
    __syncthreads();  // also: every wave is done reading h1q, the tail image may overwrite it below
    {
        const float tot = ((sm.red[0][lr] + sm.red[1][lr]) + sm.red[2][lr]) + sm.red[3][lr];
        const float meanv = tot * (1.0f / H2);
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = u[r] - __int_as_float(__builtin_amdgcn_readlane(__float_as_int(meanv), r));
        float sq[R];
#pragma unroll
        for (int r = 0; r < R; ++r) sq[r] = u[r] * u[r];
        const float s = packed_totals<R>(sq, l);
        if (l < R) sm.red2[w][l] = s;
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) sm.tail.w3s[(t + 256 * j) >> 8][(t + 256 * j) & 255] = w3r[j];
    __syncthreads();
    st = ln256_relu_store<R>(u, ln256_rstd(sm.red2, lr), nrows, p_g2, p_be2, sm.tail.h2, st);
    __syncthreads();
    COEVO_STAMP(4);

    // ---- output layer (one lane per (row, action), 256-long sequential chain out of LDS), first-max action: wave 0 ----
    if (w == 0) {
        if (l < R * NACT) {
            const int r = l / NACT, o = l % NACT;
            // (the small-launch form has registers to spare: 16 k-quads of both operands requested at a time, so that the
            // 256-step chain waits for LDS four times instead of sixteen)
            constexpr int OUT_UNROLL = FC2 == FC2_DPP ? 16 : 4;
            const float y = out_chain<OUT_UNROLL>(p_b3, &sm.tail.w3s[o][0], &sm.tail.h2[r][0]);
            sm.logit[r][o] = y;
        }
        COEVO_STAMP(5);
        // the same wave wrote the logits: a wave-level fence orders its LDS accesses, no workgroup barrier needed
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (l < nrows) {   // strict '>' scan from -inf
            const FirstMax fm = first_max_action(sm.logit[l], st);
            const int best = fm.best;
            st = fm.st;
            store_action<MODE>(a, row0 + l, best, sm.logit[l]);
        }
    }
    if (st) atomicOr(a.status, st);
    COEVO_STAMP(6);
}

}  // namespace coevo
