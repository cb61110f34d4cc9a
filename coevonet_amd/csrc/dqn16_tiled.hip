// The TILED fc1 block of the fp16 DeepQN slab (dqn16_layout.hip.h wft16; include/coevo_ext.h): its fc1 launch, pack / unpack /
// relayout and its breeding launch.  The layout of a float16 Co-GA engine, whose tasks carry 10 / 16 rows
// (HalfDQNGAEngine(fc1_layout="tiled")); the streamed form stays the default and the Co-ES layout (one row per task).
//
// Replaces, for args.precision == "float16" (reference file:line): the fc1 Linear of the half DeepQN (Atari/deepqn.py:12-37),
// AtariAgent.clone + Agent.mutate (Atari/atari_agent.py:27-30, agent.py:25-29) and the per-net half of diversity_penalty's
// np.linalg.norm (utils/game_logic_functions.py:12-37) - what dqn16.hip and dqn16_offspring.hip replace, on the other form.
//
// The float16 contract is dqn16.hip's (DESIGN.md 6a "Float16 DeepQN"): per (row, output) the sequential-k fmaf chain from the
// bias in fp32, y = f16(acc), ReLU keeps NaN.  Every weight is converted with the exact v_cvt_f32_f16 and feeds
// v_mfma_f32_16x16x4_f32 with fp32 operands (bit-identical to the sequential chain: tools/mfma16_chain_probe.hip); no f16 MFMA,
// no v_dot2, no mixed-precision FMA - their internal sums are not the sequential order.
#include "dqn_common.hip.h"
#include "dqn16_layout.hip.h"
#include "dqn16_tiled_pieces.hip.h"
#include "fc16_layout.hip.h"
#include "../../include/coevo_ext.h"

#include <type_traits>

namespace coevo {

#ifndef DQ16_FC1_TNB
#define DQ16_FC1_TNB 7   // tiled fc1: super-pieces (32 k: four 16-byte loads per lane, one per 16-output tile) in the wave's register
#endif                   // ring (98 a multiple of it): 6 x 4 KiB in flight per wave, 112 + 56 registers of weights and activations

static_assert(DQ16_SUPER == COEVO_DQN16_FC1_SUPER, "include/coevo_ext.h names the layout's constant");

typedef float f32x4_t16 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t16 __attribute__((ext_vector_type(4)));

// fc1 + ReLU of one (task, 64-output block) by one wave over the tiled block: the structure of dqn_fc1_tiled_body (deepqn.hip) -
// the wave's 64 outputs are four 16-column tiles, lane (c = l % 16, kk = l / 16), four f32x4 accumulators that start at the bias.
// Per super-piece S (32 k): four 16-byte weight loads per lane - half j of the piece of tile T IS the B operand
// B[k = 4 (8 S + j) + kk][column c] of k-quad 8 S + j, after one v_cvt_f32_f16 - two ds_read_b128 of the activations (fp32 words
// that hold fp16 values, staged per super-piece as [kk][row][j]: lane (c = row, kk) reads its eight A operands
// x[row][32 S + 4 j + kk]; pad rows are zeros) and 32 matrix instructions, k-quad by k-quad: per (row, output) the sequential-k
// chain.  A wave issues 3 136 v_mfma_f32_16x16x4 of 32 cycles on four independent accumulators (the 43 us issue floor of
// dqn_fc1_tiled_body) with one conversion each in the gap, and streams 401 408 bytes: half the fp32 kernel's.
// The ring: super-piece s lives in buffer s % NB; before it is consumed super-piece s + NB - 1 is requested.
template <int NB, bool SHARED_NET>
__device__ __forceinline__ void dqn16_fc1_tiled_body(const uint32_t *net, const DqnLayout &L, const coevo_dqn_task &task,
                                                     const float *act, float *hid, float (*xs)[4][16][8], int ob, int l)
{
    constexpr int NS = DQ16_SUPER;
    static_assert(NS % NB == 0 && NB >= 2, "whole rounds of the ring");
    const int nrows = task.n_rows, c = l & 15, kk = l >> 4;
    f32x4_t16 acc[4];
#pragma unroll
    for (int T = 0; T < 4; ++T) {
        const float bb = __uint_as_float(net[L.bf + 64 * ob + 16 * T + c]);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[T][i] = bb;
    }
    const u32x4_t16 *wp = reinterpret_cast<const u32x4_t16 *>(net + L.wf) + (size_t)ob * NS * 4 * 64 + l;
    const float *arow = act + (size_t)task.row_begin * DQ_FC1_IN;
    u32x4_t16 wv[NB][4];
    float4 xr[NB][2];
    auto issue = [&](u32x4_t16 (&w)[4], float4 (&x)[2], int S) {
#pragma unroll
        for (int T = 0; T < 4; ++T) {   // non-temporal for a net that only this task reads; plain when a neighbour shares it
            const u32x4_t16 *p = wp + (size_t)(S * 4 + T) * 64;
            if constexpr (SHARED_NET) w[T] = *p;
            else w[T] = __builtin_nontemporal_load(p);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {   // piece i: row i / 8, k-quad 8 S + i % 8 (128 bytes per row: coalesced).  A pad row requests the
            // task's last row (its zeros are put in when the piece is staged): an unconditional load, the row index a value of
            // its own, so that no exec-masked branch round the load makes the compiler's wait counts of the ring conservative
            const int i = l + 64 * j, q = i & 7;
            int r = min(i >> 3, nrows - 1);
            asm("" : "+v"(r));
            x[j] = *reinterpret_cast<const float4 *>(arow + (size_t)r * DQ_FC1_IN + 32 * S + 4 * q);
        }
    };
    // the activations of a super-piece go through LDS one super-piece AHEAD of its matrix instructions: stage() writes them,
    // fetch() reads the lane's eight A operands, and the two sit in front of and between the two halves of the previous
    // super-piece's matrix instructions, whose 1 024 issue cycles cover the LDS round trip
    auto stage = [&](const float4 (&xin)[2], float (*x_lds)[16][8]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {   // element e of k-quad 8 S + q is k = 32 S + 4 q + e: plane kk = e, slot j = q
            const int i = l + 64 * j, r = i >> 3, q = i & 7;
            const float4 v = r < nrows ? xin[j] : make_float4(0.f, 0.f, 0.f, 0.f);   // pad rows: zeros
            x_lds[0][r][q] = v.x;
            x_lds[1][r][q] = v.y;
            x_lds[2][r][q] = v.z;
            x_lds[3][r][q] = v.w;
        }
    };
    auto fetch = [&](float4 (&a)[2], float (*x_lds)[16][8]) {
        __syncthreads();   // one wave per workgroup: orders the LDS round trip
        a[0] = *reinterpret_cast<const float4 *>(&x_lds[kk][c][0]);
        a[1] = *reinterpret_cast<const float4 *>(&x_lds[kk][c][4]);
    };
    auto mfma4 = [&](const u32x4_t16 (&w)[4], const float4 &a, int half) {   // k-quads 4 half .. 4 half + 3 of the super-piece
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int T = 0; T < 4; ++T) {
                _Float16 hv[8];
                __builtin_memcpy(hv, &w[T], sizeof(hv));
                acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], (float)hv[4 * half + j], acc[T], 0, 0, 0);
            }
    };
    float4 a_cur[2], a_nxt[2];
#pragma unroll
    for (int b = 0; b < NB - 1; ++b) issue(wv[b], xr[b], b);
    stage(xr[0], xs[0]);
    fetch(a_cur, xs[0]);
    // one round of the ring.  Every request is unconditional in its instantiation - the last round (LAST) requests the one
    // super-piece that is left and nothing else - so no join of two paths makes the compiler's wait counts conservative
    auto round = [&](int s0, auto last) {
        constexpr bool LAST = decltype(last)::value;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int nb = (b + 1) % NB;
            const bool more = !LAST || b + 1 < NB;   // a super-piece follows this one
            if (!LAST || b == 0) issue(wv[(b + NB - 1) % NB], xr[(b + NB - 1) % NB], s0 + b + NB - 1);
            __builtin_amdgcn_sched_barrier(0);
            if (more) stage(xr[nb], xs[(s0 + b + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            mfma4(wv[b], a_cur[0], 0);
            __builtin_amdgcn_sched_barrier(0);
            if (more) fetch(a_nxt, xs[(s0 + b + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            mfma4(wv[b], a_cur[1], 1);
            __builtin_amdgcn_sched_barrier(0);
            a_cur[0] = a_nxt[0];
            a_cur[1] = a_nxt[1];
        }
    };
#pragma nounroll
    for (int s0 = 0; s0 < NS - NB; s0 += NB) round(s0, std::false_type{});
    round(NS - NB, std::true_type{});
#pragma unroll
    for (int T = 0; T < 4; ++T)
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // C/D of v_mfma_f32_16x16x4: column c, row 4 kk + i
            const int r = 4 * kk + i;
            if (r < nrows) hid[(size_t)(task.row_begin + r) * DQ_FC1_OUT + 64 * ob + 16 * T + c] = relu_keep_nan(f16r(acc[T][i]));
        }
}

// grid (tasks rounded up to 8, 8 output blocks), one wavefront per workgroup, one form for 1 .. 16 rows.  A task with n_rows
// outside 1 .. 16 or an unaligned net_off is reported (once, by its block 0) and skipped, as in dqn16_fc1_kernel.
// One wave per SIMD, pinned (amdgpu_waves_per_eu): at two, the 768 waves of the cfg 4 launch sometimes pair up on a SIMD, share
// its matrix pipe and take the launch from 81 to 125 us (profiles/r21_fp16_dqn_tiled_fc1.md).
template <int NB>
__global__ __launch_bounds__(64, 1) __attribute__((amdgpu_waves_per_eu(1, 1))) void dqn16_fc1_tiled_kernel(const uint32_t *slab, const coevo_dqn_task *tasks, int n_tasks, int C,
                                                                int n_actions, const float *act, float *hid, int32_t *status)
{
    __shared__ __attribute__((aligned(16))) float xs[2][4][16][8];
    // XCD x takes a contiguous range of tasks (gridDim.x is a multiple of 8), as dqn16_fc1_kernel
    const int ti = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (ti >= n_tasks) return;
    const coevo_dqn_task task = tasks[ti];
    const int ob = blockIdx.y, l = threadIdx.x;
    if (dqn16_bad_task(task)) {   // workgroup-uniform, before every barrier
        if (ob == 0 && l == 0) atomicOr(status, COEVO_ST_BAD_TASK);
        return;
    }
    // a net that acts in more than 16 games owns several tasks, adjacent in the table (workgroup-uniform)
    const bool shared_net = (ti > 0 && tasks[ti - 1].net_off == task.net_off) ||
                            (ti + 1 < n_tasks && tasks[ti + 1].net_off == task.net_off);
    const uint32_t *net = slab + task.net_off;
    const DqnLayout L = dqn16_layout(C, n_actions);
    if (shared_net) dqn16_fc1_tiled_body<NB, true>(net, L, task, act, hid, xs, ob, l);
    else dqn16_fc1_tiled_body<NB, false>(net, L, task, act, hid, xs, ob, l);
}

void dqn16_fc1_tiled_launch(const uint32_t *slab, const coevo_dqn_task *tasks, int n_tasks, int C, int n_actions, const float *act,
                            float *hid, int32_t *status, hipStream_t stream)
{
    const dim3 fg(8 * ((n_tasks + 7) / 8), 8);
    hipLaunchKernelGGL(dqn16_fc1_tiled_kernel<DQ16_FC1_TNB>, fg, dim3(64), 0, stream, slab, tasks, n_tasks, C, n_actions, act, hid,
                       status);
}

// dqn16_pack_kernel (dqn16.hip) to and from the tiled form: one thread per 32-bit word of one net's stride (blockIdx.y = net)
__global__ __launch_bounds__(256) void dqn16_pack_tiled_kernel(float *flat, uint32_t *slab, int C, int n, bool to_slab)
{
    dqn16_pack_word(flat, slab, C, n, to_slab, 1);
}

// dst (fc1 form dst_tiled) := src (fc1 form src_tiled), one thread per 32-bit word of one net's stride: a word of the fc1 block
// gathers its two halves from their places in the other form, every other word - the padding included - is copied
__global__ __launch_bounds__(256) void dqn16_relayout_kernel(const uint32_t *src, uint32_t *dst, int C, int n, int src_tiled,
                                                              int dst_tiled)
{
    const DqnLayout L = dqn16_layout(C, n);
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= L.stride) return;
    const uint32_t *sn = src + (int64_t)blockIdx.y * L.stride;
    uint32_t *dn = dst + (int64_t)blockIdx.y * L.stride;
    if (s < L.wf || s >= L.bf || src_tiled == dst_tiled) {
        dn[s] = sn[s];
        return;
    }
    const uint16_t *sh = reinterpret_cast<const uint16_t *>(sn + L.wf);
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int64_t f = dqn16_fc1_half_to_flat(2 * (s - L.wf) + e, dst_tiled);
        w |= (uint32_t)sh[dqn16_fc1_flat_to_half(f / DQ_FC1_IN, f % DQ_FC1_IN, src_tiled)] << (16 * e);
    }
    dn[s] = w;
}

// grid (coevo_dqn16_perturb_blocks, n_children): dq16_perturb_dist_body (dqn16_pieces.hip.h) with the tiled fc1 block's noise -
// the thread -> piece map, the blocks of 256 pieces and the fp64 order of the distance terms are dqn16_perturb_dist_kernel's
__global__ __launch_bounds__(256) void dqn16_perturb_dist_tiled_kernel(Dq16PerturbArgs a)
{
    __shared__ double scratch[4];
    dq16_perturb_dist_body(a, scratch, [](int u, const DqnLayout &L, int C, float sigma, uint64_t seed, uint32_t slo, uint32_t shi,
                                          float (&noise)[8]) { dq16_fc1_piece_noise_tiled(u, L, C, sigma, seed, slo, shi, noise); });
}

}  // namespace coevo

using namespace coevo;

static int dqn16_pack_tiled_launch(float *flat, uint32_t *slab, int n, int C, int n_actions, bool to_slab, void *stream)
{
    if (!flat || !slab || n <= 0 || !dqn_shape_ok(C, n_actions)) return COEVO_ERR_ARG;
    const dim3 grid((unsigned)((dqn16_layout(C, n_actions).stride + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(dqn16_pack_tiled_kernel, grid, dim3(256), 0, (hipStream_t)stream, flat, slab, C, n_actions, to_slab);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn16_pack_tiled(const float *flat, void *slab, int n, int C, int n_actions, void *stream)
{
    return dqn16_pack_tiled_launch(const_cast<float *>(flat), static_cast<uint32_t *>(slab), n, C, n_actions, true, stream);
}

extern "C" int coevo_dqn16_unpack_tiled(const void *slab, float *flat, int n, int C, int n_actions, void *stream)
{
    return dqn16_pack_tiled_launch(flat, const_cast<uint32_t *>(static_cast<const uint32_t *>(slab)), n, C, n_actions, false, stream);
}

extern "C" int coevo_dqn16_relayout(const void *src, void *dst, int n, int C, int n_actions, int src_tiled, int dst_tiled,
                                    void *stream)
{
    if (!src || !dst || src == dst || !aligned16(src) || !aligned16(dst)) return COEVO_ERR_ARG;
    if (n < 0 || n > 65535 || !dqn_shape_ok(C, n_actions)) return COEVO_ERR_ARG;   // (any bit or-ed into C fails here)
    if ((src_tiled & ~1) || (dst_tiled & ~1)) return COEVO_ERR_ARG;
    if (n == 0) return COEVO_OK;
    const dim3 grid((unsigned)((dqn16_layout(C, n_actions).stride + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(dqn16_relayout_kernel, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const uint32_t *>(src),
                       static_cast<uint32_t *>(dst), C, n_actions, src_tiled, dst_tiled);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn16_perturb_dist_tiled(const void *parent_slab, const int32_t *parent_idx, void *child_slab, int child_first,
                                              int n_children, int C, int n_actions, const float *sigma_dev, uint64_t seed,
                                              uint32_t stream_lo_first, uint32_t stream_hi, int flags, const int32_t *gen_dev,
                                              int gen_bias, const void *dist_ref, double *dist_partial, void *stream)
{
    const int rc = dqn16_perturb_args(parent_slab, parent_idx, child_slab, child_first, n_children, C, n_actions, sigma_dev, flags,
                                      dist_ref, dist_partial);
    if (rc != COEVO_OK) return rc < 0 ? rc : COEVO_OK;
    const Dq16PerturbArgs a{static_cast<const uint32_t *>(parent_slab), parent_idx, static_cast<uint32_t *>(child_slab), child_first,
                            C, n_actions, sigma_dev, seed, stream_lo_first, stream_hi, flags, gen_dev, gen_bias,
                            static_cast<const uint32_t *>(dist_ref), dist_partial};
    hipLaunchKernelGGL(dqn16_perturb_dist_tiled_kernel, dim3(dqn16_blocks(C, n_actions), (unsigned)n_children), dim3(256), 0,
                       (hipStream_t)stream, a);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
