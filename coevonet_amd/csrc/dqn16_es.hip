// Float16 Co-ES update on the fp16 DeepQN slab of dqn16_layout.hip.h: the noise-regenerating chunk sums and the update of the
// base net.  The fitness is coevo_es16_fitness (fc16_es.hip: its rewards[game * 3 + slot] addressing is SynthRollout.acc's).
//
// Replaces, for args.precision == "float16" (reference file:line): compute_weight_update (evolutionary_strategy.py:120-148)
// on the half arrays that mutate_weights collected (:63-116, get_numpy_dtype(args.precision) :71-74) and base_weights +=
// update (:259-265), for the layers DeepQN.get_perturbable_layers names (Atari/deepqn.py:158-172: every conv and Linear
// weight and bias; nn.BatchNorm2d is skipped).  As at the top of fc16_es.hip: the reference multiplies the STORED noise, rounded
// to half, and f16(f32(theta) + noise) - theta (coevo_dqn_es_partial's route) is not that noise.  The partial kernel therefore
// draws every individual's Philox noise again, piece by piece exactly as dqn16_perturb_dist_kernel (dqn16_offspring.hip) walks
// the net, rounds it to fp16 and accumulates it against the fitness.  No noise matrix is stored and no perturbed net is read.
//
// The float16 DeepQN Co-ES contract (DESIGN.md 6a "Float16 DeepQN Co-ES"):
//   noise16[j][p]  f16(sigma * eps(seed, stream_lo_first + j, stream_hi, p)), the product rounded to fp32 first, p the canonical
//                  parameters() index: the numbers coevo_dqn16_perturb_dist(COEVO_DQP_SKIP_BN) added for that stream; conv and
//                  Linear weights and biases only; round to nearest even, fp16 subnormals kept
//   sum            chunk c = individuals [c n / C, (c + 1) n / C), j ascending, acc = fmaf(f32(fit16[j]), f32(noise16[j][p]), acc)
//                  from 0 in fp32; chunk sums added left to right in fp32; dot16 = f16(sum), past 65504 inf
//   apply          scale16 = f16(lr / (n sigma)) (fp64 quotient, one rounding), upd16 = f16(f32(scale16) f32(dot16)),
//                  theta' = f16(f32(theta) + f32(upd16)); BatchNorm affine and padding keep their words
// A thread owns ONE 16-byte piece of the net: in the fc1 block eight halves = two aligned Philox quads, everywhere else four
// fp32 words that hold fp16 values and map through dqn16_word_to_flat (a conv piece can need four Philox blocks; the last one
// drawn is kept).
#include <hip/hip_runtime.h>

#include "dqn16_layout.hip.h"
#include "fc16_pieces.hip.h"
#include "philox.hip.h"

namespace coevo {

// A chunk partial, in floats: the net's entries in slab order, every half entry widened to one float - the words in front of
// fc1 as they are, 8 floats per fc1 piece, then one float per word up to the stride (0 at BatchNorm and padding words).
__host__ __device__ inline int64_t dq16es_partial_floats(const DqnLayout &L) { return L.stride + DQ16_FC1_WORDS; }
__host__ __device__ inline int64_t dq16es_piece_float(int u, const DqnLayout &L)
{
    const int64_t s = 4 * (int64_t)u;
    return s < L.wf ? s : (s < L.bf ? L.wf + 2 * (s - L.wf) : s + DQ16_FC1_WORDS);
}

__device__ __forceinline__ int dq16es_pieces(const DqnLayout &L) { return (int)(L.stride >> 2); }
__device__ __forceinline__ bool dq16es_fc1_piece(int u, const DqnLayout &L)
{
    return 4 * (int64_t)u >= L.wf && 4 * (int64_t)u < L.bf;
}
// word s outside the fc1 block moves in an update: a parameter, and not BatchNorm affine
__device__ __forceinline__ bool dq16es_word_moves(int64_t s, const DqnLayout &L)
{
    return s < L.total && !dqn_slab_is_batchnorm(s, L);
}

// Left alone, hipcc folds a multiply or an add into the conversion that follows it (v_fma_mix*: the exact result rounded once
// to fp16), which skips the fp32 rounding of the contract.  The empty statement makes the fp32 value a value of its own
// (es16_noise16 of fc16_es.hip, dq16_pin of dqn16_offspring.hip).
__device__ __forceinline__ float dq16es_pin(float v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// noise16 = f16(noise32), noise32 = sigma * eps the fp32 number the perturb launch added; the converted value is pinned too, so
// the fmaf that consumes it is a plain fp32 one
__device__ __forceinline__ float dq16es_noise16(float noise32) { return dq16es_pin(f16r(dq16es_pin(noise32))); }

// grid (coevo_dqn16_perturb_blocks, chunks_total): workgroup (bx, c) sums pieces 256 bx .. 256 bx + 255 over chunk c's individuals
__global__ __launch_bounds__(256) void dqn16_es_partial_kernel(int C, int n_actions, const float *fitness, int n_total,
                                                                int chunks_total, const float *sigma_dev, uint64_t seed,
                                                                uint32_t stream_lo_first, uint32_t stream_hi, float *partial)
{
    const DqnLayout L = dqn16_layout(C, n_actions);
    const int u = blockIdx.x * 256 + (int)threadIdx.x;
    if (u >= dq16es_pieces(L)) return;
    const int c = blockIdx.y;
    const int j_lo = (int)((int64_t)c * n_total / chunks_total), j_hi = (int)((int64_t)(c + 1) * n_total / chunks_total);
    const float sigma = *sigma_dev;
    float *out = partial + (int64_t)c * dq16es_partial_floats(L) + dq16es_piece_float(u, L);
    if (dq16es_fc1_piece(u, L)) {
        // piece (ob, o, l) = fc1.w[64 ob + l][8 o .. 8 o + 7]: never BatchNorm, never padding
        const int t = u - (int)(L.wf >> 2), l = t & 63, o = (t >> 6) % DQ16_OCTETS, ob = (t >> 6) / DQ16_OCTETS;
        const int F_wf = 2048 * C + 69792;   // conv1.w conv1.b conv2.w conv2.b conv3.w conv3.b come first
        const uint32_t q0 = (uint32_t)((F_wf + (ob * 64 + l) * DQ_FC1_IN + 8 * o) >> 2);
        float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = j_lo; j < j_hi; ++j) {
            const uint32_t slo = stream_lo_first + (uint32_t)j;
            float z[8];
            philox_normal4(seed, slo, stream_hi, q0, z);
            philox_normal4(seed, slo, stream_hi, q0 + 1u, z + 4);
            const float f = fitness[j];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(f, dq16es_noise16(sigma * z[i]), acc[i]);
        }
        reinterpret_cast<float4 *>(out)[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        reinterpret_cast<float4 *>(out)[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
        // the four words' canonical indices do not depend on the individual: mapped once, in front of the loop
        int64_t p[4];
        bool moves[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t s = 4 * (int64_t)u + i;
            moves[i] = dq16es_word_moves(s, L);
            p[i] = moves[i] ? dqn16_word_to_flat(s, C, n_actions) : -1;
        }
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (moves[0] || moves[1] || moves[2] || moves[3]) {
            for (int j = j_lo; j < j_hi; ++j) {
                const uint32_t slo = stream_lo_first + (uint32_t)j;
                const float f = fitness[j];
                float zz[4];
                int64_t have = -1;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (!moves[i]) continue;
                    const int64_t q = p[i] >> 2;
                    if (q != have) { philox_normal4(seed, slo, stream_hi, (uint32_t)q, zz); have = q; }
                    const int e = (int)(p[i] & 3);
                    const float zi = e == 0 ? zz[0] : (e == 1 ? zz[1] : (e == 2 ? zz[2] : zz[3]));   // (no runtime-indexed array)
                    acc[i] = __builtin_fmaf(f, dq16es_noise16(sigma * zi), acc[i]);
                }
            }
        }
        reinterpret_cast<float4 *>(out)[0] = make_float4(moves[0] ? acc[0] : 0.0f, moves[1] ? acc[1] : 0.0f,
                                                         moves[2] ? acc[2] : 0.0f, moves[3] ? acc[3] : 0.0f);
    }
}

// theta' = f16(theta + f16(scale16 * f16(p_0 + p_1 + ... left to right))): every fp32 intermediate a value of its own
__device__ __forceinline__ float dq16es_new_theta(float theta, float sum, float scale16)
{
    const float dot16 = dq16es_pin(f16r(dq16es_pin(sum)));
    const float upd16 = dq16es_pin(f16r(dq16es_pin(scale16 * dot16)));
    return f16r(dq16es_pin(dq16es_pin(theta) + upd16));
}

__global__ __launch_bounds__(256) void dqn16_es_apply_kernel(uint32_t *theta, const float *partial, int chunks_total, int C,
                                                              int n_actions, int n_total, const float *sigma_dev, double lr)
{
    const DqnLayout L = dqn16_layout(C, n_actions);
    const int u = blockIdx.x * 256 + (int)threadIdx.x;
    if (u >= dq16es_pieces(L)) return;
    const float scale16 = f16_of_f64(lr / ((double)n_total * (double)*sigma_dev));
    const float *pp = partial + dq16es_piece_float(u, L);
    const int64_t pitch = dq16es_partial_floats(L);
    const uint4 tv = reinterpret_cast<const uint4 *>(theta)[u];
    uint4 ov;
    if (dq16es_fc1_piece(u, L)) {
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
        for (int i = 0; i < 8; ++i) hout[i] = (_Float16)dq16es_new_theta((float)hin[i], sum[i], scale16);
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
            out[i] = dq16es_word_moves(4 * (int64_t)u + i, L) ? dq16es_new_theta(in[i], sum[i], scale16) : in[i];
        __builtin_memcpy(&ov, out, sizeof(out));
    }
    reinterpret_cast<uint4 *>(theta)[u] = ov;
}

}  // namespace coevo

using namespace coevo;

constexpr int DQ16ES_MAX_CHUNKS = 64;

static unsigned dq16es_blocks(int C, int n) { return quad_blocks(dqn16_layout(C, n).stride); }

extern "C" int64_t coevo_dqn_es16_partial_floats(int C, int n_actions)
{
    return dqn_shape_ok(C, n_actions) ? dq16es_partial_floats(dqn16_layout(C, n_actions)) : COEVO_ERR_ARG;
}

extern "C" int coevo_dqn_es16_partial(int C, int n_actions, const float *fitness, int n_total, int chunks_total,
                                      const float *sigma_dev, uint64_t seed, uint32_t stream_lo_first, uint32_t stream_hi,
                                      float *partial, void *stream)
{
    if (!fitness || !sigma_dev || !partial || n_total < 1) return COEVO_ERR_ARG;
    if (!dqn_shape_ok(C, n_actions)) return COEVO_ERR_ARG;   // (any bit or-ed into C fails here)
    if (chunks_total < 1 || chunks_total > DQ16ES_MAX_CHUNKS || !aligned16(partial)) return COEVO_ERR_ARG;
    const dim3 grid(dq16es_blocks(C, n_actions), (unsigned)chunks_total);
    hipLaunchKernelGGL(dqn16_es_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, C, n_actions, fitness, n_total,
                       chunks_total, sigma_dev, seed, stream_lo_first, stream_hi, partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn_es16_apply(void *theta16_net, const float *partial, int chunks_total, int C, int n_actions,
                                    int n_total, const float *sigma_dev, double lr, void *stream)
{
    if (!theta16_net || !partial || !sigma_dev || n_total < 1) return COEVO_ERR_ARG;
    if (!dqn_shape_ok(C, n_actions)) return COEVO_ERR_ARG;
    if (chunks_total < 1 || chunks_total > DQ16ES_MAX_CHUNKS) return COEVO_ERR_ARG;
    if (!aligned16(theta16_net) || !aligned16(partial)) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(dqn16_es_apply_kernel, dim3(dq16es_blocks(C, n_actions)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<uint32_t *>(theta16_net), partial, chunks_total, C, n_actions, n_total, sigma_dev, lr);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
