// Float16 Co-ES update on the fp16 slab of fc16_layout.hip.h: the fitness in half, the noise-regenerating chunk sums and the
// update of the base net.
//
// Replaces, for args.precision == "float16" (reference file:line): compute_weight_update (evolutionary_strategy.py:120-148)
// on the half arrays that mutate_weights collected (:63-116: mutate_ES(...).astype(np.float16), agent.py:31-70) and
// base_weights += update (:259-265).  The reference multiplies the STORED noise, rounded to half; the perturbed net is
// f16(f32(theta) + noise), so pert - theta (coevo_es_partial's route) is not that noise.  The partial kernel therefore draws
// every individual's Philox noise again, through f16_half_piece_noise / f16_tail_piece_noise of fc16_pieces.hip.h - the
// functions the perturbed nets were written with -, rounds it to fp16 and accumulates it against the fitness.  No noise
// matrix is stored and no perturbed net is read.
//
// The float16 Co-ES contract (DESIGN.md 6a "Float16 Co-ES"):
//   noise16[j][p]  f16(sigma * eps(seed, stream_lo_first + j, stream_hi, p)), the product rounded to fp32 first; Linear weights
//                  and biases only; round to nearest even, fp16 subnormals kept
//   fit16[j]       f16(reward_j) in ONE rounding from fp64; with a sharing score f16(f32(fit16[j]) / (1.0f + score))
//   sum            chunk c = individuals [c n / C, (c + 1) n / C), j ascending, acc = fmaf(f32(fit16[j]), f32(noise16[j][p]), acc)
//                  from 0 in fp32; chunk sums added left to right in fp32; dot16 = f16(sum), past 65504 inf
//   apply          scale16 = f16(lr / (n sigma)) (fp64 quotient, one rounding), upd16 = f16(f32(scale16) f32(dot16)),
//                  theta' = f16(f32(theta) + f32(upd16)); LayerNorm affine and padding keep their words
// A thread owns ONE 16-byte piece of the net, as in fc16_perturb_dist_kernel.
#include <hip/hip_runtime.h>

#include "coevo_common.hip.h"
#include "fc16_layout.hip.h"
#include "fc16_pieces.hip.h"
#include "philox.hip.h"

namespace coevo {

// A chunk partial, in floats: the net's entries in slab order, every half entry widened to one float - 8 floats per piece of
// W2h / W1h / W3h, then one float per word of the fp32 tail up to the stride (0 at LayerNorm and padding words).
__host__ __device__ constexpr int64_t es16_partial_floats(int D) { return 2 * f16_off_b1(D) + (f16_stride(D) - f16_off_b1(D)); }
__host__ __device__ constexpr int64_t es16_piece_float(int u, int D)
{
    return u < f16_half_pieces(D) ? 8 * (int64_t)u : 2 * f16_off_b1(D) + 4 * (int64_t)(u - f16_half_pieces(D));
}

// noise16 = f16(noise32).  noise32 = sigma * eps is the fp32 number the perturb launch added, so it is rounded to fp32 BEFORE it
// is rounded to fp16.  Left alone, the compiler folds the multiply into the conversion that feeds the mixed-precision fmaf
// (v_fma_mixlo_f16: the exact product rounded once to fp16), which differs from the contract at about one entry in 10^5.  The
// empty statement makes the fp32 product a value of its own.
__device__ __forceinline__ float es16_noise16(float noise32)
{
    asm volatile("" : "+v"(noise32));
    return f16r(noise32);
}

// fitness[j] = f16(rewards[game_idx[j]][slot]) [ / (1 + *score), rounded again ]
__global__ __launch_bounds__(256) void es16_fitness_kernel(const double *rewards, const int32_t *game_idx, int slot, int n,
                                                            const float *score, float *fitness)
{
    const int j = blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= n) return;
    float f = f16_of_f64(rewards[(int64_t)game_idx[j] * 3 + slot]);
    if (score) f = f16r(f / (1.0f + *score));
    fitness[j] = f;
}

// grid (f16_perturb_blocks(D), chunks_total): workgroup (bx, c) sums pieces 256 bx .. 256 bx + 255 over chunk c's individuals
__global__ __launch_bounds__(256) void fc16_es_partial_kernel(int D, const float *fitness, int n_total, int chunks_total,
                                                               const float *sigma_dev, uint64_t seed,
                                                               uint32_t stream_lo_first, uint32_t stream_hi, float *partial)
{
    const int u = blockIdx.x * 256 + (int)threadIdx.x;
    if (u >= f16_pieces(D)) return;
    const int c = blockIdx.y;
    const int j_lo = (int)((int64_t)c * n_total / chunks_total), j_hi = (int)((int64_t)(c + 1) * n_total / chunks_total);
    const float sigma = *sigma_dev;
    float *out = partial + (int64_t)c * es16_partial_floats(D) + es16_piece_float(u, D);
    if (u < f16_half_pieces(D)) {
        float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = j_lo; j < j_hi; ++j) {
            float noise[8];
            f16_half_piece_noise(u, D, sigma, seed, stream_lo_first + (uint32_t)j, stream_hi, noise);
            const float f = fitness[j];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(f, es16_noise16(noise[i]), acc[i]);
        }
        reinterpret_cast<float4 *>(out)[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        reinterpret_cast<float4 *>(out)[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool bias[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bias[i] = f16_tail_kind(4 * u + i, D) == 0;
        if (bias[0] || bias[1] || bias[2] || bias[3]) {
            for (int j = j_lo; j < j_hi; ++j) {
                float noise[4];
                f16_tail_piece_noise(u, D, sigma, seed, stream_lo_first + (uint32_t)j, stream_hi, noise);
                const float f = fitness[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(f, es16_noise16(noise[i]), acc[i]);
            }
        }
        reinterpret_cast<float4 *>(out)[0] = make_float4(bias[0] ? acc[0] : 0.0f, bias[1] ? acc[1] : 0.0f,
                                                         bias[2] ? acc[2] : 0.0f, bias[3] ? acc[3] : 0.0f);
    }
}

// theta' = f16(theta + f16(scale16 * f16(p_0 + p_1 + ... left to right))) on piece u of the base net
__device__ __forceinline__ float es16_new_theta(float theta, float sum, float scale16)
{
    const float dot16 = f16r(sum);
    const float upd16 = f16r(scale16 * dot16);
    return f16r(theta + upd16);
}

__global__ __launch_bounds__(256) void fc16_es_apply_kernel(uint32_t *theta, const float *partial, int chunks_total, int D,
                                                             int n_total, const float *sigma_dev, double lr)
{
    const int u = blockIdx.x * 256 + (int)threadIdx.x;
    if (u >= f16_pieces(D)) return;
    const float scale16 = f16_of_f64(lr / ((double)n_total * (double)*sigma_dev));
    const float *pp = partial + es16_piece_float(u, D);
    const int64_t pitch = es16_partial_floats(D);
    const uint4 tv = reinterpret_cast<const uint4 *>(theta)[u];
    uint4 ov;
    if (u < f16_half_pieces(D)) {
        float4 lo = reinterpret_cast<const float4 *>(pp)[0], hi = reinterpret_cast<const float4 *>(pp)[1];
        for (int c = 1; c < chunks_total; ++c) {
            const float4 a = reinterpret_cast<const float4 *>(pp + c * pitch)[0];
            const float4 b = reinterpret_cast<const float4 *>(pp + c * pitch)[1];
            lo.x = lo.x + a.x; lo.y = lo.y + a.y; lo.z = lo.z + a.z; lo.w = lo.w + a.w;
            hi.x = hi.x + b.x; hi.y = hi.y + b.y; hi.z = hi.z + b.z; hi.w = hi.w + b.w;
        }
        const float sum[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        _Float16 hin[8], hout[8];
        __builtin_memcpy(hin, &tv, sizeof(hin));
#pragma unroll
        for (int i = 0; i < 8; ++i) hout[i] = (_Float16)es16_new_theta((float)hin[i], sum[i], scale16);
        __builtin_memcpy(&ov, hout, sizeof(hout));
    } else {
        float4 t = reinterpret_cast<const float4 *>(pp)[0];
        for (int c = 1; c < chunks_total; ++c) {
            const float4 a = reinterpret_cast<const float4 *>(pp + c * pitch)[0];
            t.x = t.x + a.x; t.y = t.y + a.y; t.z = t.z + a.z; t.w = t.w + a.w;
        }
        const float sum[4] = {t.x, t.y, t.z, t.w};
        float in[4], out[4];
        __builtin_memcpy(in, &tv, sizeof(in));
#pragma unroll
        for (int i = 0; i < 4; ++i)
            out[i] = f16_tail_kind(4 * u + i, D) == 0 ? es16_new_theta(in[i], sum[i], scale16) : in[i];
        __builtin_memcpy(&ov, out, sizeof(out));
    }
    reinterpret_cast<uint4 *>(theta)[u] = ov;
}

}  // namespace coevo

using namespace coevo;

constexpr int ES16_MAX_CHUNKS = 64;

extern "C" int64_t coevo_es16_partial_floats(int D) { return fc_dim_ok(D) ? es16_partial_floats(D) : COEVO_ERR_ARG; }

extern "C" int coevo_es16_fitness(const double *rewards, const int32_t *game_idx, int slot, int n, const float *score,
                                  float *fitness, void *stream)
{
    if (!rewards || !game_idx || !fitness || slot < 0 || slot > 2 || n < 1) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(es16_fitness_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rewards,
                       game_idx, slot, n, score, fitness);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_es16_partial(int D, const float *fitness, int n_total, int chunks_total, const float *sigma_dev,
                                  uint64_t seed, uint32_t stream_lo_first, uint32_t stream_hi, float *partial, void *stream)
{
    if (!fitness || !sigma_dev || !partial || !fc_dim_ok(D) || n_total < 1) return COEVO_ERR_ARG;
    if (chunks_total < 1 || chunks_total > ES16_MAX_CHUNKS || !aligned16(partial)) return COEVO_ERR_ARG;
    const dim3 grid((unsigned)f16_perturb_blocks(D), (unsigned)chunks_total);
    hipLaunchKernelGGL(fc16_es_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, D, fitness, n_total, chunks_total,
                       sigma_dev, seed, stream_lo_first, stream_hi, partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_es16_apply(void *theta16_net, const float *partial, int chunks_total, int D, int n_total,
                                const float *sigma_dev, double lr, void *stream)
{
    if (!theta16_net || !partial || !sigma_dev || !fc_dim_ok(D) || n_total < 1) return COEVO_ERR_ARG;
    if (chunks_total < 1 || chunks_total > ES16_MAX_CHUNKS) return COEVO_ERR_ARG;
    if (!aligned16(theta16_net) || !aligned16(partial)) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(fc16_es_apply_kernel, dim3((unsigned)f16_perturb_blocks(D)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<uint32_t *>(theta16_net), partial, chunks_total, D, n_total, sigma_dev, lr);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
