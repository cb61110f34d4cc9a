// DeepQN in float16 (args.precision == "float16", reference Atari/deepqn.py:12-37: every conv, Linear and BatchNorm module is
// half): the fp16 slab, its pack / unpack, and the policy forward + first-max action of coevo_dqn16_forward_argmax.
//
// The float16 contract (DESIGN.md 6a "Float16 DeepQN"): the canonical fp32 arithmetic of deepqn.hip / oracle/coevo_oracle.c
// with fp16 storage and one fp16 rounding wherever the reference's half module rounds:
//   x       = f16(u8 / 255)  (the correctly rounded fp32 quotient, rounded once)
//   conv    acc = bias; acc = fmaf(w, x, acc) over the taps in (ci, ky, kx) order in fp32; y = f16(acc)
//   BatchNorm (training mode, batch 1) the canonical fp32 rule on the fp16 sums, output f16; ReLU keeps NaN
//   fc1 / output  sequential-k fmaf chain from the bias in fp32, y = f16(acc); ReLU after fc1
//   action  the first maximum of a strict '>' scan over the fp16 logits; COEVO_ST_NO_ACTION when no logit compares
// Three launches, the structure of the fp32 forward:
//   dqn16_conv_kernel  one workgroup per frame: conv16_mfma / bn_relu_rows of dqn_conv.hip.h with H16 = true (LDS keeps fp32
//                      words that hold fp16 values: the fp32 kernel's footprint, three workgroups per CU)
//   dqn16_fc1_kernel   one wave per (task, 64-output block) streams the block's 2-byte weights once per task
//   dqn16_out_kernel   512 -> n logits, rounded to fp16, first-max action (dqn_out_row<true>, dqn_common.hip.h)
// coevo_dqn16_forward_hidden stops after the second: a rollout runs the output row inside its env-step launch
// (coevo_dqn16_out_synth_step, dqn_engine.hip), as the float32 rollout does.
// Weights are converted with the exact v_cvt_f32_f16 and feed fp32 chains (v_mfma_f32_4x4x1 / 16x16x4 with fp32 operands are
// bit-identical to the sequential fmaf chain: tools/mfma4_chain_probe.hip, tools/mfma16_chain_probe.hip); no f16 MFMA, no
// v_dot2, no mixed-precision FMA - their internal sums are not the sequential order.
#include "dqn_common.hip.h"
#include "dqn_conv.hip.h"
#include "dqn16_layout.hip.h"
#include "fc16_layout.hip.h"
#include "../../include/coevo_ext.h"

namespace coevo {

#ifndef DQ16_FC1_U
#define DQ16_FC1_U 7     // fc1: k-octets (16-byte pieces of 8 halves) per chunk of the weight stream (392 = 56 x 7)
#endif
#ifndef DQ16_FC1_NB
#define DQ16_FC1_NB 8    // fc1: chunks in the wave's register ring (NB - 1 in flight: 7 x 7 KiB, the fp32 kernel's bytes)
#endif

// one thread per 32-bit word of one net's stride (blockIdx.y = net).  to_slab: every entry is rounded to fp16 to nearest even
// (exact for fp16 values; the reference's .to(float16)), the padding is zeroed.  Else slab -> flat (fp16 values as fp32).
__global__ __launch_bounds__(256) void dqn16_pack_kernel(float *flat, uint32_t *slab, int C, int n, bool to_slab)
{
    dqn16_pack_word(flat, slab, C, n, to_slab, 0);
}

// The conv stack of one frame: dqn_conv_kernel (deepqn.hip) with the contract's three rounding points.  One form serves every
// row count.  A frame of a task the forward cannot serve writes nothing (the test is uniform over the workgroup and comes
// before every barrier).
template <int CMAX, int CT>
__global__ __launch_bounds__(512, DQ_WPE) void dqn16_conv_kernel(const uint32_t *slab, const coevo_dqn_task *tasks, int n_tasks,
                                                             int n_rows, int C, int n_actions, const uint8_t *frames, float *act)
{
    __shared__ __attribute__((aligned(16))) DqnSmem<CMAX> sm;
    const int per = gridDim.x >> 3;   // XCD x takes the contiguous rows [x * per, (x + 1) * per): a net's frames meet in one L2
    const int row = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (row >= n_rows) return;   // workgroup-uniform (the grid is rounded up to a multiple of 8)
    const coevo_dqn_task task = tasks[task_of_row(tasks, n_tasks, row)];
    if (dqn16_bad_task(task)) return;
    const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(t >> 6), l = t & 63;
    const float *net = reinterpret_cast<const float *>(slab + task.net_off);   // the sections in front of fc1: fp32 words
    const DqnLayout L = dqn16_layout(C, n_actions);
    const int nbytes = 84 * 84 * C;   // a multiple of 16
    const uint4 *src = reinterpret_cast<const uint4 *>(frames + (size_t)row * nbytes);
    uint4 *dst = reinterpret_cast<uint4 *>(sm.frame);
    for (int i = t; i < nbytes / 16; i += 512) dst[i] = src[i];
    if (DQ_LUT && t < 256) sm.lut[t] = (float)t / 255.0f;
    __syncthreads();
    conv16_mfma<8, 4, 84, 20, 32, true, 0, DQ_P1, CT, DQ_QU1, true, true>(sm.frame, sm.lut, C, C * 64, net + L.w1, net + L.b1, sm.a1, w, l);
    __syncthreads();
    bn_relu_rows<400, DQ_P1, 32, true>(sm.a1, net + L.b1 + 32, net + L.b1 + 64, w, l);
    __syncthreads();
    conv16_mfma<4, 2, 20, 9, 64, false, DQ_P1, DQ_P2, 0, DQ_QU2, true, true>(sm.a1, nullptr, 32, 512, net + L.w2, net + L.b2, sm.a2, w, l);
    __syncthreads();
    bn_relu_rows<81, DQ_P2, 64, true>(sm.a2, net + L.b2 + 64, net + L.b2 + 128, w, l);
    __syncthreads();
    conv16_mfma<3, 1, 9, 7, 64, false, DQ_P2, DQ_P3, 0, DQ_QU3, false, true>(sm.a2, nullptr, 64, 576, net + L.w3, net + L.b3, sm.a3, w, l);
    __syncthreads();
    bn_relu_rows<49, DQ_P3, 64, true>(sm.a3, net + L.b3 + 64, net + L.b3 + 128, w, l);
    __syncthreads();
    // flatten in CHW order (Atari/deepqn.py:45): channel pitch 49 = the flat layout itself
    float *dsta = act + (size_t)row * DQ_FC1_IN;
    for (int i = t; i < DQ_FC1_IN; i += 512) dsta[i] = sm.a3[i];
}

constexpr int DQ16_RMAX = COEVO_DQN_MAX_ROWS;
typedef float f32x4_acc16 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_w16 __attribute__((ext_vector_type(4)));

// fc1 + ReLU of one (task, 64-output block) by one wave: lane l owns output 64 ob + l and streams its row as 16-byte pieces of
// eight halves, each read exactly once per task (non-temporal: nothing of the 3.2 MB per net is worth a cache line).  Rows
// in groups of four on v_mfma_f32_4x4x1_16B_f32, the form of dqn_fc1_body: the A operand x[4g + l % 4][k] comes from the
// chunk's activations staged in LDS (one ds_read_b128 per group and four k), the B operand is the lane's own weight
// converted by v_cvt_f32_f16, C-in = the bias: per (row, output) the sequential-k fp32 chain.  NG = ceil(rows / 4).
// The ring: chunk c lives in buffer c % NB; before chunk c is consumed chunk c + NB - 1 is requested.
template <int NG, int NB>
__device__ __forceinline__ void dqn16_fc1_body(const uint32_t *net, const DqnLayout &L, const coevo_dqn_task &task,
                                               const float *act, float *hid, float (*xs)[DQ16_RMAX][DQ16_FC1_U * 8], int ob, int l)
{
    constexpr int U = DQ16_FC1_U, NCHUNK = DQ16_OCTETS / U, PR = 2 * U;   // PR: float4 activation pieces per row and chunk
    static_assert(DQ16_OCTETS % U == 0 && NCHUNK % NB == 0 && NB >= 2 && NB % 2 == 0, "whole rounds of the ring");
    static_assert(4 * NG <= DQ16_RMAX, "rows of one task");
    const int nrows = task.n_rows, col = 64 * ob + l;
    const float bb = __uint_as_float(net[L.bf + col]);
    f32x4_acc16 acc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[g][i] = bb;
    const u32x4_w16 *wp = reinterpret_cast<const u32x4_w16 *>(net + L.wf) + (size_t)ob * DQ16_OCTETS * 64 + l;
    const float *arow = act + (size_t)task.row_begin * DQ_FC1_IN;
    constexpr int XI = (4 * NG * PR + 63) / 64;
    u32x4_w16 wv[NB][U];
    float4 xr[NB][XI];
    auto issue = [&](u32x4_w16 (&w)[U], float4 (&x)[XI], int c) {
#pragma unroll
        for (int u = 0; u < U; ++u) w[u] = __builtin_nontemporal_load(wp + (size_t)(c * U + u) * 64);
#pragma unroll
        for (int j = 0; j < XI; ++j) {   // piece i: row i / PR, floats 4 (i % PR) .. + 3 of the chunk (coalesced per row; pad rows: zeros)
            const int i = l + 64 * j, r = i / PR, q = i % PR;
            x[j] = (i < 4 * NG * PR && r < nrows)
                       ? *reinterpret_cast<const float4 *>(arow + (size_t)r * DQ_FC1_IN + 8 * U * c + 4 * q)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto consume = [&](const u32x4_w16 (&w)[U], const float4 (&xin)[XI], float (*x_lds)[DQ16_FC1_U * 8]) {
#pragma unroll
        for (int j = 0; j < XI; ++j) {
            const int i = l + 64 * j;
            if (i < 4 * NG * PR) *reinterpret_cast<float4 *>(&x_lds[i / PR][4 * (i % PR)]) = xin[j];
        }
        __syncthreads();   // one wave per workgroup: orders the LDS round trip
        // the broadcast reads of the next four k are requested before the matrix instructions of these four are issued (two
        // register sets, the order pinned), as in dqn_fc1_body
        float4 x[2][NG];
        auto read_x = [&](float4 (&dst)[NG], int hq) {
#pragma unroll
            for (int g = 0; g < NG; ++g) dst[g] = *reinterpret_cast<const float4 *>(&x_lds[4 * g + (l & 3)][4 * hq]);
        };
        read_x(x[0], 0);
#pragma unroll
        for (int hq = 0; hq < 2 * U; ++hq) {   // four k per step: half of a 16-byte weight piece
            if (hq + 1 < 2 * U) read_x(x[(hq + 1) & 1], hq + 1);
            __builtin_amdgcn_sched_barrier(0);
            _Float16 hv[8];
            __builtin_memcpy(hv, &w[hq >> 1], sizeof(hv));
            const float b0 = (float)hv[4 * (hq & 1)], b1 = (float)hv[4 * (hq & 1) + 1], b2 = (float)hv[4 * (hq & 1) + 2],
                        b3 = (float)hv[4 * (hq & 1) + 3];
            const float4 (&xc)[NG] = x[hq & 1];
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(xc[g].x, b0, acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(xc[g].y, b1, acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(xc[g].z, b2, acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(xc[g].w, b3, acc[g], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
#pragma unroll
    for (int b = 0; b < NB - 1; ++b) issue(wv[b], xr[b], b);
#pragma nounroll
    for (int c0 = 0; c0 < NCHUNK; c0 += NB) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int nxt = c0 + b + NB - 1;
            if (nxt < NCHUNK) issue(wv[(b + NB - 1) % NB], xr[(b + NB - 1) % NB], nxt);   // wave-uniform
            __builtin_amdgcn_sched_barrier(0);
            consume(wv[b], xr[b], xs[b & 1]);
        }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * g + i;
            if (r < nrows) hid[(size_t)(task.row_begin + r) * DQ_FC1_OUT + col] = relu_keep_nan(f16r(acc[g][i]));
        }
}

// grid (tasks rounded up to 8, 8 output blocks), one wavefront per workgroup.  A task with n_rows outside 1 .. 16 or an
// unaligned net_off is reported (once, by its block 0) and skipped.
__global__ __launch_bounds__(64, 1) void dqn16_fc1_kernel(const uint32_t *slab, const coevo_dqn_task *tasks, int n_tasks, int C,
                                                          int n_actions, const float *act, float *hid, int32_t *status)
{
    __shared__ __attribute__((aligned(16))) float xs[2][DQ16_RMAX][DQ16_FC1_U * 8];
    // XCD x takes a contiguous range of tasks (gridDim.x is a multiple of 8), as dqn_fc1_kernel
    const int ti = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (ti >= n_tasks) return;
    const coevo_dqn_task task = tasks[ti];
    const int ob = blockIdx.y, l = threadIdx.x;
    if (dqn16_bad_task(task)) {   // workgroup-uniform, before every barrier
        if (ob == 0 && l == 0) atomicOr(status, COEVO_ST_BAD_TASK);
        return;
    }
    const uint32_t *net = slab + task.net_off;
    const DqnLayout L = dqn16_layout(C, n_actions);
    const int ng = (task.n_rows + 3) >> 2;   // workgroup-uniform: one straight-line instantiation each
    if (ng == 1) dqn16_fc1_body<1, DQ16_FC1_NB>(net, L, task, act, hid, xs, ob, l);
    else if (ng == 2) dqn16_fc1_body<2, DQ16_FC1_NB>(net, L, task, act, hid, xs, ob, l);
    else if (ng == 3) dqn16_fc1_body<3, DQ16_FC1_NB>(net, L, task, act, hid, xs, ob, l);
    else dqn16_fc1_body<4, DQ16_FC1_NB>(net, L, task, act, hid, xs, ob, l);
}

// output layer + first-max action: one 64-thread workgroup per row runs dqn_out_row<true> (dqn_common.hip.h), the one body of
// the float16 output row - the fused env step of dqn_engine.hip (coevo_dqn16_out_synth_step) runs the same
__global__ __launch_bounds__(64) void dqn16_out_kernel(const uint32_t *slab, const coevo_dqn_task *tasks, int n_tasks, int C,
                                                        int n_actions, const float *hid, int32_t *actions, float *logits,
                                                        int32_t *status)
{
    __shared__ __attribute__((aligned(16))) float xs[DQ_FC1_OUT];
    __shared__ float lg[64];
    const int row = blockIdx.x, tid = threadIdx.x;
    const coevo_dqn_task task = tasks[task_of_row(tasks, n_tasks, row)];
    if (dqn16_bad_task(task)) return;   // workgroup-uniform, before every barrier: the row is left untouched
    const float *net = reinterpret_cast<const float *>(slab + task.net_off);
    const int a = dqn_out_row<true>(net, dqn16_layout(C, n_actions), n_actions, hid + (size_t)row * DQ_FC1_OUT,
                                    logits ? logits + (size_t)row * COEVO_DQN_LOGIT_STRIDE : nullptr, status, xs, lg, tid);
    if (tid == 0) actions[row] = a;
}

}  // namespace coevo

using namespace coevo;


extern "C" int64_t coevo_dqn16_slab_stride(int C, int n_actions)
{
    return dqn_shape_ok(C, n_actions) ? dqn16_layout(C, n_actions).stride : COEVO_ERR_ARG;
}

extern "C" int64_t coevo_dqn16_workspace_bytes(int n_rows_total)
{
    return n_rows_total > 0 ? (int64_t)n_rows_total * (DQ_FC1_IN + DQ_FC1_OUT) * 4 : COEVO_ERR_ARG;
}

static int dqn16_pack_launch(float *flat, uint32_t *slab, int n, int C, int n_actions, bool to_slab, void *stream)
{
    if (!flat || !slab || n <= 0 || !dqn_shape_ok(C, n_actions)) return COEVO_ERR_ARG;
    const dim3 grid((unsigned)((dqn16_layout(C, n_actions).stride + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(dqn16_pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, flat, slab, C, n_actions, to_slab);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn16_pack(const float *flat, void *slab, int n, int C, int n_actions, void *stream)
{
    return dqn16_pack_launch(const_cast<float *>(flat), static_cast<uint32_t *>(slab), n, C, n_actions, true, stream);
}

extern "C" int coevo_dqn16_unpack(const void *slab, float *flat, int n, int C, int n_actions, void *stream)
{
    return dqn16_pack_launch(flat, const_cast<uint32_t *>(static_cast<const uint32_t *>(slab)), n, C, n_actions, false, stream);
}

// conv stack + fc1 of every row (hid: post-ReLU fc1 outputs, fp16 values, behind the conv3 activations in the workspace), after
// the argument checks the float16 forward entry points share.  fc1_tiled: the slab's fc1 block is wft16 (dqn16_layout.hip.h; the
// *_tiled entry points of include/coevo_ext.h) and the fc1 launch is dqn16_tiled.hip's
static int dqn16_hidden_launch(const void *slab, const coevo_dqn_task *tasks, int n_tasks, int max_rows_per_task, int n_rows_total,
                               int C, int n_actions, const uint8_t *frames, int32_t *status, void *workspace, hipStream_t s,
                               bool fc1_tiled)
{
    if (!slab || !tasks || !frames || !status || !workspace) return COEVO_ERR_ARG;
    if (n_tasks <= 0 || n_rows_total <= 0 || !dqn_shape_ok(C, n_actions)) return COEVO_ERR_ARG;   // (any bit or-ed into C fails here)
    if (max_rows_per_task < 1 || max_rows_per_task > DQ16_RMAX) return COEVO_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(slab) & 15) return COEVO_ERR_ARG;
    const uint32_t *sl = static_cast<const uint32_t *>(slab);
    float *act = static_cast<float *>(workspace);
    float *hid = act + (size_t)n_rows_total * DQ_FC1_IN;
    const dim3 cg(8 * ((n_rows_total + 7) / 8)), cb(512);   // a multiple of 8: the kernel's XCD-aware row mapping
    if (C == 4) hipLaunchKernelGGL((dqn16_conv_kernel<4, 4>), cg, cb, 0, s, sl, tasks, n_tasks, n_rows_total, C, n_actions, frames, act);
    else if (C < 4) hipLaunchKernelGGL((dqn16_conv_kernel<4, 0>), cg, cb, 0, s, sl, tasks, n_tasks, n_rows_total, C, n_actions, frames, act);
    else if (C == 6) hipLaunchKernelGGL((dqn16_conv_kernel<6, 6>), cg, cb, 0, s, sl, tasks, n_tasks, n_rows_total, C, n_actions, frames, act);
    else hipLaunchKernelGGL((dqn16_conv_kernel<6, 0>), cg, cb, 0, s, sl, tasks, n_tasks, n_rows_total, C, n_actions, frames, act);
    const dim3 fg(8 * ((n_tasks + 7) / 8), 8);
    if (fc1_tiled) dqn16_fc1_tiled_launch(sl, tasks, n_tasks, C, n_actions, act, hid, status, s);
    else hipLaunchKernelGGL(dqn16_fc1_kernel, fg, dim3(64), 0, s, sl, tasks, n_tasks, C, n_actions, act, hid, status);
    return COEVO_OK;
}

static int dqn16_argmax_launch(const void *slab, const coevo_dqn_task *tasks, int n_tasks, int max_rows_per_task, int n_rows_total,
                               int C, int n_actions, const uint8_t *frames, int32_t *actions, float *logits, int32_t *status,
                               void *workspace, void *stream, bool fc1_tiled)
{
    if (!actions) return COEVO_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int rc = dqn16_hidden_launch(slab, tasks, n_tasks, max_rows_per_task, n_rows_total, C, n_actions, frames, status,
                                       workspace, s, fc1_tiled);
    if (rc != COEVO_OK) return rc;
    const float *hid = static_cast<const float *>(workspace) + (size_t)n_rows_total * DQ_FC1_IN;
    hipLaunchKernelGGL(dqn16_out_kernel, dim3(n_rows_total), dim3(64), 0, s, static_cast<const uint32_t *>(slab), tasks, n_tasks, C,
                       n_actions, hid, actions, logits, status);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

static int dqn16_hidden_checked(const void *slab, const coevo_dqn_task *tasks, int n_tasks, int max_rows_per_task, int n_rows_total,
                                int C, int n_actions, const uint8_t *frames, int32_t *status, void *workspace, void *stream,
                                bool fc1_tiled)
{
    const int rc = dqn16_hidden_launch(slab, tasks, n_tasks, max_rows_per_task, n_rows_total, C, n_actions, frames, status,
                                       workspace, (hipStream_t)stream, fc1_tiled);
    if (rc != COEVO_OK) return rc;
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn16_forward_argmax(const void *slab, const coevo_dqn_task *tasks, int n_tasks, int max_rows_per_task,
                                          int n_rows_total, int C, int n_actions, const uint8_t *frames, int32_t *actions,
                                          float *logits, int32_t *status, void *workspace, void *stream)
{
    return dqn16_argmax_launch(slab, tasks, n_tasks, max_rows_per_task, n_rows_total, C, n_actions, frames, actions, logits,
                               status, workspace, stream, false);
}

extern "C" int coevo_dqn16_forward_hidden(const void *slab, const coevo_dqn_task *tasks, int n_tasks, int max_rows_per_task,
                                          int n_rows_total, int C, int n_actions, const uint8_t *frames, int32_t *status,
                                          void *workspace, void *stream)
{
    return dqn16_hidden_checked(slab, tasks, n_tasks, max_rows_per_task, n_rows_total, C, n_actions, frames, status, workspace,
                                stream, false);
}

// ---- the same two over a slab whose fc1 block is TILED (include/coevo_ext.h): the conv launch and the output launch are the
// ones above, the fc1 launch is dqn16_fc1_tiled_kernel (dqn16_tiled.hip); arguments and refusals are their twins'
extern "C" int coevo_dqn16_forward_argmax_tiled(const void *slab, const coevo_dqn_task *tasks, int n_tasks, int max_rows_per_task,
                                                int n_rows_total, int C, int n_actions, const uint8_t *frames, int32_t *actions,
                                                float *logits, int32_t *status, void *workspace, void *stream)
{
    return dqn16_argmax_launch(slab, tasks, n_tasks, max_rows_per_task, n_rows_total, C, n_actions, frames, actions, logits,
                               status, workspace, stream, true);
}

extern "C" int coevo_dqn16_forward_hidden_tiled(const void *slab, const coevo_dqn_task *tasks, int n_tasks, int max_rows_per_task,
                                                int n_rows_total, int C, int n_actions, const uint8_t *frames, int32_t *status,
                                                void *workspace, void *stream)
{
    return dqn16_hidden_checked(slab, tasks, n_tasks, max_rows_per_task, n_rows_total, C, n_actions, frames, status, workspace,
                                stream, true);
}
