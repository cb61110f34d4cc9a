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
// A thread owns ONE 16-byte piece of the net, as in fc16_perturb_dist_kernel.  The roundings are f16_noise16 / f16_new_theta
// of fc16_layout.hip.h; the accumulate, the chunk totals and the argument checks are those of f16_steps.hip.h.
#include <hip/hip_runtime.h>

#include "f16_steps.hip.h"
#include "fc16_pieces.hip.h"

namespace coevo {

// A chunk partial, in floats: the net's entries in slab order, every half entry widened to one float - 8 floats per piece of
// W2h / W1h / W3h, then one float per word of the fp32 tail up to the stride (0 at LayerNorm and padding words).
__host__ __device__ constexpr int64_t es16_partial_floats(int D) { return 2 * f16_off_b1(D) + (f16_stride(D) - f16_off_b1(D)); }
__host__ __device__ constexpr int64_t es16_piece_float(int u, int D)
{
    return u < f16_half_pieces(D) ? 8 * (int64_t)u : 2 * f16_off_b1(D) + 4 * (int64_t)(u - f16_half_pieces(D));
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
            f16_es_accumulate(acc, fitness[j], noise);
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
                f16_es_accumulate(acc, fitness[j], noise);
            }
        }
        reinterpret_cast<float4 *>(out)[0] = make_float4(bias[0] ? acc[0] : 0.0f, bias[1] ? acc[1] : 0.0f,
                                                         bias[2] ? acc[2] : 0.0f, bias[3] ? acc[3] : 0.0f);
    }
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
        float sum[8];
        f16_chunk_total8(pp, pitch, chunks_total, sum);
        ov = f16_apply_halves(tv, sum, scale16);
    } else {
        float sum[4];
        bool moves[4];
        f16_chunk_total4(pp, pitch, chunks_total, sum);
#pragma unroll
        for (int i = 0; i < 4; ++i) moves[i] = f16_tail_kind(4 * u + i, D) == 0;
        ov = f16_apply_words(tv, sum, scale16, moves);
    }
    reinterpret_cast<uint4 *>(theta)[u] = ov;
}

}  // namespace coevo

using namespace coevo;

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
    if (!es16_partial_args_ok(fitness, sigma_dev, partial, fc_dim_ok(D), n_total, chunks_total)) return COEVO_ERR_ARG;
    const dim3 grid((unsigned)f16_perturb_blocks(D), (unsigned)chunks_total);
    hipLaunchKernelGGL(fc16_es_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, D, fitness, n_total, chunks_total,
                       sigma_dev, seed, stream_lo_first, stream_hi, partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_es16_apply(void *theta16_net, const float *partial, int chunks_total, int D, int n_total,
                                const float *sigma_dev, double lr, void *stream)
{
    if (!es16_apply_args_ok(theta16_net, partial, sigma_dev, fc_dim_ok(D), n_total, chunks_total)) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(fc16_es_apply_kernel, dim3((unsigned)f16_perturb_blocks(D)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<uint32_t *>(theta16_net), partial, chunks_total, D, n_total, sigma_dev, lr);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
