// FCNetwork in float16 (args.precision == "float16", reference MPE/fcnetwork.py:13): the weight slab, its pack / unpack,
// and the policy forward + first-max action of coevo_fc16_forward_argmax.
//
// The float16 contract (DESIGN.md "float16 nets"): the canonical fp32 arithmetic of coevo_common.hip.h with fp16 storage
// and fp16 rounding points, following where the reference's torch-CPU half forward rounds:
//   x     = f16(obs)
//   Linear  acc = b[j]; acc = fmaf(w[j][k], x[k], acc) for k = 0..K-1 in fp32 (w, x fp16 values: every product is exact),
//           y = f16(acc) (round to nearest even; past 65504 -> inf)
//   LayerNorm the canonical fp32 rule on the fp16 inputs (gamma / beta stay fp32), output rounded to fp16; ReLU
//   logits  fp16 values; the action is the first maximum of a strict '>' scan (ties are common in fp16)
//   status  COEVO_ST_* bits as in fp32, tested on the rounded values
// Weights are converted to fp32 on load (v_cvt_f32_f16, exact) and fed to plain v_fmac_f32 chains: no f16 MFMA and no
// v_dot2, whose internal sums are not the sequential order.
#include <hip/hip_runtime.h>

#include "coevo_common.hip.h"
#include "fc16_layout.hip.h"

namespace coevo {

// canonical flat index p (torch parameters() order, the fp32 slab's section offsets) -> place in the fp16 slab:
// returns the HALF index for a Linear weight (*is_half = true), else the fp32 WORD index
__device__ inline int64_t f16_place(int64_t p, int D, bool *is_half)
{
    *is_half = true;
    if (p < fc_off_b1(D)) {                         // fc1.w[j][k] -> W1h[k][j]
        const int64_t j = p / D, k = p % D;
        return 2 * F16_W1 + k * H1 + j;
    }
    if (p >= fc_off_w2(D) && p < fc_off_b2(D)) {    // fc2.w[j][k] -> W2h[k / 8][j][k % 8]
        const int64_t t = p - fc_off_w2(D), j = t / H1, k = t % H1;
        return ((k >> 3) * H2 + j) * 8 + (k & 7);
    }
    if (p >= fc_off_w3(D) && p < fc_off_b3(D))      // output.w[o][k] -> W3h[o][k]
        return 2 * f16_off_w3(D) + (p - fc_off_w3(D));
    *is_half = false;
    if (p < fc_off_w2(D)) return f16_off_b1(D) + (p - fc_off_b1(D));
    if (p < fc_off_w3(D)) return f16_off_b2(D) + (p - fc_off_b2(D));
    return f16_off_b3(D) + (p - fc_off_b3(D));
}

// one thread per flat entry of one net (blockIdx.y); the threads past the last entry zero the stride's padding words
__global__ __launch_bounds__(256) void fc16_pack_kernel(const float *flat, uint32_t *slab, int D, bool to_slab)
{
    const int64_t net = blockIdx.y, P = fc_params(D), stride = f16_stride(D);
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t *s = slab + net * stride;
    if (p >= P) {
        const int64_t pad = f16_used(D) + (p - P);
        if (to_slab && pad < stride) s[pad] = 0u;
        return;
    }
    bool is_half;
    const int64_t q = f16_place(p, D, &is_half);
    float *f = const_cast<float *>(flat) + net * P + p;
    if (to_slab) {
        // Linear entries round to nearest even (exact for fp16 values); a bias is stored upcast, the LayerNorm affine as is
        const bool bias = (p >= fc_off_b1(D) && p < fc_off_b1(D) + H1) || (p >= fc_off_b2(D) && p < fc_off_b2(D) + H2) ||
                          p >= fc_off_b3(D);
        if (is_half) reinterpret_cast<_Float16 *>(s)[q] = (_Float16)*f;
        else reinterpret_cast<float *>(s)[q] = bias ? (float)(_Float16)*f : *f;
    } else {
        *f = is_half ? (float)reinterpret_cast<const _Float16 *>(s)[q] : reinterpret_cast<const float *>(s)[q];
    }
}


struct Fc16Args {
    const uint32_t *slab;
    const coevo_fc_task *tasks;
    const float *obs;
    int32_t *actions;
    float *logits;
    int32_t *status;
};

// One workgroup = one task.  fc1: thread t owns outputs t and t + 256; fc2: thread t owns output column t and streams its
// 64 pieces (8 k each); each LayerNorm row is reduced by one wave with the canonical packed butterfly; the output layer is
// one thread per (row, action).  Activations (fp16 values held as fp32) live in LDS and are read as broadcasts.
__global__ __launch_bounds__(256) void fc16_policy_kernel(Fc16Args a)
{
    __shared__ float xs[F16_R][16];
    __shared__ float h1[F16_R][H1];
    __shared__ float h2[F16_R][H2];
    __shared__ float lg[F16_R][8];
    __shared__ int st_sh;
    const coevo_fc_task task = a.tasks[blockIdx.x];
    const int D = task.D;
    // a task this kernel cannot serve (the W2h pieces are 16-byte loads: net_off must be a multiple of 4 words) is skipped
    // and reported; the test is uniform over the workgroup
    if ((D != 8 && D != 10) || task.n_rows < 1 || task.n_rows > COEVO_FC_MAX_ROWS || (task.net_off & 3) != 0) {
        if (threadIdx.x == 0) atomicOr(a.status, COEVO_ST_BAD_TASK);
        return;
    }
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const uint32_t *net = a.slab + task.net_off;
    const uint4 *W2 = reinterpret_cast<const uint4 *>(net);
    const _Float16 *W1 = reinterpret_cast<const _Float16 *>(net + F16_W1);
    const _Float16 *W3 = reinterpret_cast<const _Float16 *>(net + f16_off_w3(D));
    const float *b1 = reinterpret_cast<const float *>(net + f16_off_b1(D)), *g1 = b1 + H1, *be1 = b1 + 2 * H1;
    const float *b2 = reinterpret_cast<const float *>(net + f16_off_b2(D)), *g2 = b2 + H2, *be2 = b2 + 2 * H2;
    const float *b3 = reinterpret_cast<const float *>(net + f16_off_b3(D));
    if (t == 0) st_sh = 0;
    int st = 0;
    for (int rg = 0; rg < task.n_rows; rg += F16_R) {
        const int nr = min(F16_R, task.n_rows - rg);
        __syncthreads();   // the previous pass is done with the LDS rows
        if (t < F16_R * 16) {
            const int r = t >> 4, k = t & 15;
            float v = 0.0f;
            if (r < nr && k < D) {
                v = f16r(a.obs[(int64_t)(task.row_begin + rg + r) * COEVO_OBS_STRIDE + k]);
                if (!__builtin_isfinite(v)) st |= COEVO_ST_BAD_INPUT;
            }
            xs[r][k] = v;
        }
        __syncthreads();
        // fc1 (K = D)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int j = t + 256 * hh;
            float wk[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) wk[k] = (k < D) ? (float)W1[k * H1 + j] : 0.0f;
            const float b = b1[j];
#pragma unroll
            for (int r = 0; r < F16_R; ++r) {
                float acc = b;
#pragma unroll
                for (int k = 0; k < 10; ++k)
                    if (k < D) acc = __builtin_fmaf(wk[k], xs[r][k], acc);
                h1[r][j] = f16r(acc);
            }
        }
        __syncthreads();
        // LayerNorm(512) + ReLU: wave w takes rows w, w + 4
        for (int r = w; r < nr; r += 4) {
            float v[8], q[8];
#pragma unroll
            for (int b = 0; b < 8; ++b) v[b] = h1[r][64 * b + l];
            const float mean = row_blocks_total<8>(v, l) * (1.0f / H1);
#pragma unroll
            for (int b = 0; b < 8; ++b) { v[b] = v[b] - mean; q[b] = v[b] * v[b]; }
            const float var = row_blocks_total<8>(q, l) * (1.0f / H1);
            const float rstd = 1.0f / __builtin_sqrtf(var + LN_EPS);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int j = 64 * b + l;
                const float y = f16r(__builtin_fmaf(v[b] * rstd, g1[j], be1[j]));
                if (bad_post_relu16(y)) st |= COEVO_ST_BAD_FC1;
                h1[r][j] = (y > 0.0f) ? y : (__builtin_isnan(y) ? y : 0.0f);
            }
        }
        __syncthreads();
        // fc2 (K = 512): column t, 64 pieces of 8 k
        {
            float acc[F16_R];
            const float b = b2[t];
#pragma unroll
            for (int r = 0; r < F16_R; ++r) acc[r] = b;
            for (int kb = 0; kb < H1 / 8; ++kb) {
                const uint4 piece = W2[kb * H2 + t];
                _Float16 hv[8];
                __builtin_memcpy(hv, &piece, sizeof(hv));
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const float wv = (float)hv[kk];
#pragma unroll
                    for (int r = 0; r < F16_R; ++r) acc[r] = __builtin_fmaf(wv, h1[r][8 * kb + kk], acc[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < F16_R; ++r) h2[r][t] = f16r(acc[r]);
        }
        __syncthreads();
        // LayerNorm(256) + ReLU
        for (int r = w; r < nr; r += 4) {
            float v[4], q[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) v[b] = h2[r][64 * b + l];
            const float mean = row_blocks_total<4>(v, l) * (1.0f / H2);
#pragma unroll
            for (int b = 0; b < 4; ++b) { v[b] = v[b] - mean; q[b] = v[b] * v[b]; }
            const float var = row_blocks_total<4>(q, l) * (1.0f / H2);
            const float rstd = 1.0f / __builtin_sqrtf(var + LN_EPS);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = 64 * b + l;
                const float y = f16r(__builtin_fmaf(v[b] * rstd, g2[j], be2[j]));
                if (bad_post_relu16(y)) st |= COEVO_ST_BAD_FC2;
                h2[r][j] = (y > 0.0f) ? y : (__builtin_isnan(y) ? y : 0.0f);
            }
        }
        __syncthreads();
        // output layer (K = 256): one thread per (row, action)
        if (t < NACT * F16_R) {
            const int o = t % NACT, r = t / NACT;
            float acc = b3[o];
            for (int k = 0; k < H2; ++k) acc = __builtin_fmaf((float)W3[o * H2 + k], h2[r][k], acc);
            lg[r][o] = f16r(acc);
        }
        __syncthreads();
        if (t < nr) {
            const int row = task.row_begin + rg + t;
            int best = -1;
            float cur = -__builtin_inff();
#pragma unroll
            for (int o = 0; o < NACT; ++o) {
                const float v = lg[t][o];
                if (!__builtin_isfinite(v)) st |= COEVO_ST_BAD_OUT;
                if (v > cur) { cur = v; best = o; }
            }
            if (best < 0) { st |= COEVO_ST_NO_ACTION; best = 0; }
            a.actions[row] = best;
            if (a.logits) {
#pragma unroll
                for (int o = 0; o < NACT; ++o) a.logits[(int64_t)row * COEVO_LOGIT_STRIDE + o] = lg[t][o];
            }
        }
    }
    if (st) atomicOr(&st_sh, st);
    __syncthreads();
    if (t == 0 && st_sh) atomicOr(a.status, st_sh);
}

}  // namespace coevo

using namespace coevo;

extern "C" int64_t coevo_fc16_slab_stride(int D) { return fc_dim_ok(D) ? f16_stride(D) : COEVO_ERR_ARG; }

static int fc16_pack_launch(const float *flat, uint32_t *slab, int n, int D, bool to_slab, void *stream)
{
    if (!flat || !slab || n <= 0 || !fc_dim_ok(D)) return COEVO_ERR_ARG;
    const int64_t threads = fc_params(D) + (f16_stride(D) - f16_used(D));
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(fc16_pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, flat, slab, D, to_slab);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc16_pack(const float *flat, void *slab, int n, int D, void *stream)
{
    return fc16_pack_launch(flat, static_cast<uint32_t *>(slab), n, D, true, stream);
}

extern "C" int coevo_fc16_unpack(const void *slab, float *flat, int n, int D, void *stream)
{
    return fc16_pack_launch(flat, const_cast<uint32_t *>(static_cast<const uint32_t *>(slab)), n, D, false, stream);
}

extern "C" int coevo_fc16_forward_argmax(const void *slab, const coevo_fc_task *tasks, int n_tasks, int max_rows_per_task,
                                         const float *obs, int32_t *actions, float *logits, int32_t *status, void *stream)
{
    if (!slab || !tasks || !obs || !actions || !status || n_tasks < 0) return COEVO_ERR_ARG;
    if (max_rows_per_task < 1 || max_rows_per_task > COEVO_FC_MAX_ROWS) return COEVO_ERR_ARG;
    if (n_tasks == 0) return COEVO_OK;
    const Fc16Args a{static_cast<const uint32_t *>(slab), tasks, obs, actions, logits, status};
    hipLaunchKernelGGL(fc16_policy_kernel, dim3((unsigned)n_tasks), dim3(256), 0, (hipStream_t)stream, a);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
