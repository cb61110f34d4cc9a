// Float16 Co-ES update on the fp16 DeepQN slab of dqn16_layout.hip.h: the noise-regenerating chunk sums and the update of the
// base net.  The fitness is coevo_es16_fitness (fc16_es.hip: its rewards[game * 3 + slot] addressing is SynthRollout.acc's).
//
// Replaces, for args.precision == "float16" (reference file:line): compute_weight_update (evolutionary_strategy.py:120-148)
// on the half arrays that mutate_weights collected (:63-116, get_numpy_dtype(args.precision) :71-74) and base_weights +=
// update (:259-265), for the layers DeepQN.get_perturbable_layers names (Atari/deepqn.py:158-172: every conv and Linear
// weight and bias; nn.BatchNorm2d is skipped).  As at the top of fc16_es.hip: the reference multiplies the STORED noise, rounded
// to half, and f16(f32(theta) + noise) - theta (coevo_dqn_es_partial's route) is not that noise.  The partial kernel therefore
// draws every individual's Philox noise again, through dq16_fc1_piece_noise / dq16_word_piece_noise of dqn16_pieces.hip.h - the
// functions dqn16_perturb_dist_kernel (dqn16_offspring.hip) wrote the perturbed nets with -, rounds it to fp16 and accumulates
// it against the fitness.  No noise matrix is stored and no perturbed net is read.
//
// The float16 DeepQN Co-ES contract (DESIGN.md 6a "Float16 DeepQN Co-ES"):
//   noise16[j][p]  f16(sigma * eps(seed, stream_lo_first + j, stream_hi, p)), the product rounded to fp32 first, p the canonical
//                  parameters() index: the numbers coevo_dqn16_perturb_dist(COEVO_DQP_SKIP_BN) added for that stream; conv and
//                  Linear weights and biases only; round to nearest even, fp16 subnormals kept
//   sum            chunk c = individuals [c n / C, (c + 1) n / C), j ascending, acc = fmaf(f32(fit16[j]), f32(noise16[j][p]), acc)
//                  from 0 in fp32; chunk sums added left to right in fp32; dot16 = f16(sum), past 65504 inf
//   apply          scale16 = f16(lr / (n sigma)) (fp64 quotient, one rounding), upd16 = f16(f32(scale16) f32(dot16)),
//                  theta' = f16(f32(theta) + f32(upd16)); BatchNorm affine and padding keep their words
// A thread owns ONE 16-byte piece of the net, as in dqn16_perturb_dist_kernel.  The roundings are f16_noise16 / f16_new_theta
// of fc16_layout.hip.h; the accumulate, the chunk totals and the argument checks are those of f16_steps.hip.h.
#include <hip/hip_runtime.h>

#include "dqn16_pieces.hip.h"
#include "f16_steps.hip.h"

namespace coevo {

// A chunk partial, in floats: the net's entries in slab order, every half entry widened to one float - the words in front of
// fc1 as they are, 8 floats per fc1 piece, then one float per word up to the stride (0 at BatchNorm and padding words).
__host__ __device__ inline int64_t dqn16_partial_floats(const DqnLayout &L) { return L.stride + DQ16_FC1_WORDS; }
__host__ __device__ inline int64_t dqn16_piece_float(int u, const DqnLayout &L)
{
    const int64_t s = 4 * (int64_t)u;
    return s < L.wf ? s : (s < L.bf ? L.wf + 2 * (s - L.wf) : s + DQ16_FC1_WORDS);
}

// grid (coevo_dqn16_perturb_blocks, chunks_total): workgroup (bx, c) sums pieces 256 bx .. 256 bx + 255 over chunk c's individuals
__global__ __launch_bounds__(256) void dqn16_es_partial_kernel(int C, int n_actions, const float *fitness, int n_total,
                                                                int chunks_total, const float *sigma_dev, uint64_t seed,
                                                                uint32_t stream_lo_first, uint32_t stream_hi, float *partial)
{
    const DqnLayout L = dqn16_layout(C, n_actions);
    const int u = blockIdx.x * 256 + (int)threadIdx.x;
    if (u >= dq16_pieces(L)) return;
    const int c = blockIdx.y;
    const int j_lo = (int)((int64_t)c * n_total / chunks_total), j_hi = (int)((int64_t)(c + 1) * n_total / chunks_total);
    const float sigma = *sigma_dev;
    float *out = partial + (int64_t)c * dqn16_partial_floats(L) + dqn16_piece_float(u, L);
    if (dq16_fc1_piece(u, L)) {
        float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = j_lo; j < j_hi; ++j) {
            float noise[8];
            dq16_fc1_piece_noise(u, L, C, sigma, seed, stream_lo_first + (uint32_t)j, stream_hi, noise);
            f16_es_accumulate(acc, fitness[j], noise);
        }
        reinterpret_cast<float4 *>(out)[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        reinterpret_cast<float4 *>(out)[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
        // a parameter that is not BatchNorm affine moves (COEVO_DQP_SKIP_BN's words)
        int64_t p[4];
        bool moves[4];
        dq16_word_piece_flat(u, C, n_actions, p);
#pragma unroll
        for (int i = 0; i < 4; ++i) moves[i] = dq16_word_moves(4 * (int64_t)u + i, L, true);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (moves[0] || moves[1] || moves[2] || moves[3]) {
            for (int j = j_lo; j < j_hi; ++j) {
                float noise[4];
                dq16_word_piece_noise(p, moves, sigma, seed, stream_lo_first + (uint32_t)j, stream_hi, noise);
                f16_es_accumulate(acc, fitness[j], noise);
            }
        }
        reinterpret_cast<float4 *>(out)[0] = make_float4(moves[0] ? acc[0] : 0.0f, moves[1] ? acc[1] : 0.0f,
                                                         moves[2] ? acc[2] : 0.0f, moves[3] ? acc[3] : 0.0f);
    }
}

__global__ __launch_bounds__(256) void dqn16_es_apply_kernel(uint32_t *theta, const float *partial, int chunks_total, int C,
                                                              int n_actions, int n_total, const float *sigma_dev, double lr)
{
    const DqnLayout L = dqn16_layout(C, n_actions);
    const int u = blockIdx.x * 256 + (int)threadIdx.x;
    if (u >= dq16_pieces(L)) return;
    const float scale16 = f16_of_f64(lr / ((double)n_total * (double)*sigma_dev));
    const float *pp = partial + dqn16_piece_float(u, L);
    const int64_t pitch = dqn16_partial_floats(L);
    const uint4 tv = reinterpret_cast<const uint4 *>(theta)[u];
    uint4 ov;
    if (dq16_fc1_piece(u, L)) {
        float sum[8];
        f16_chunk_total8(pp, pitch, chunks_total, sum);
        ov = f16_apply_halves(tv, sum, scale16);
    } else {
        float sum[4];
        bool moves[4];
        f16_chunk_total4(pp, pitch, chunks_total, sum);
#pragma unroll
        for (int i = 0; i < 4; ++i) moves[i] = dq16_word_moves(4 * (int64_t)u + i, L, true);
        ov = f16_apply_words(tv, sum, scale16, moves);
    }
    reinterpret_cast<uint4 *>(theta)[u] = ov;
}

}  // namespace coevo

using namespace coevo;

extern "C" int64_t coevo_dqn_es16_partial_floats(int C, int n_actions)
{
    return dqn_shape_ok(C, n_actions) ? dqn16_partial_floats(dqn16_layout(C, n_actions)) : COEVO_ERR_ARG;
}

extern "C" int coevo_dqn_es16_partial(int C, int n_actions, const float *fitness, int n_total, int chunks_total,
                                      const float *sigma_dev, uint64_t seed, uint32_t stream_lo_first, uint32_t stream_hi,
                                      float *partial, void *stream)
{
    // (any bit or-ed into C fails dqn_shape_ok)
    if (!es16_partial_args_ok(fitness, sigma_dev, partial, dqn_shape_ok(C, n_actions), n_total, chunks_total)) return COEVO_ERR_ARG;
    const dim3 grid(dqn16_blocks(C, n_actions), (unsigned)chunks_total);
    hipLaunchKernelGGL(dqn16_es_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, C, n_actions, fitness, n_total,
                       chunks_total, sigma_dev, seed, stream_lo_first, stream_hi, partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn_es16_apply(void *theta16_net, const float *partial, int chunks_total, int C, int n_actions,
                                    int n_total, const float *sigma_dev, double lr, void *stream)
{
    if (!es16_apply_args_ok(theta16_net, partial, sigma_dev, dqn_shape_ok(C, n_actions), n_total, chunks_total)) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(dqn16_es_apply_kernel, dim3(dqn16_blocks(C, n_actions)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<uint32_t *>(theta16_net), partial, chunks_total, C, n_actions, n_total, sigma_dev, lr);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
