// Float16 Co-GA breeding on the fp16 DeepQN slab of dqn16_layout.hip.h: offspring with their stale-agent distance fused in, and
// the distance of nets that are already in a slab.  The finalize is coevo_fc16_distance_finalize (fc16_offspring.hip: its
// n_blocks is generic); gather, HoF push and elites are coevo_net_gather with the stride in words.
//
// Replaces, for args.precision == "float16" (reference file:line): AtariAgent.clone + Agent.mutate (Atari/atari_agent.py:27-30,
// agent.py:25-29: half_param.data += torch.normal(0, sigma, size) for EVERY parameter - the BatchNorm affine is half in
// DeepQN, Atari/deepqn.py:24-37) and np.linalg.norm(a16 - b16) of diversity_penalty on get_weights_ES() = all parameters
// (utils/game_logic_functions.py:12-37).
//
// The float16 DeepQN breeding contract (DESIGN.md 6a "Float16 DeepQN breeding"):
//   mutation   child = f16(f32(parent) + noise), noise = sigma * eps(seed, stream, p) rounded to fp32 first, p the canonical
//              parameters() index (coevo_dqn_param_count's order): the number the fp32 child of the same stream draws
//              (coevo_dqn_perturb).  Round to nearest even, past 65504 -> inf, fp16 subnormals kept.
//   distance   per entry d = f16(f32(a) - f32(b)); d * d accumulated in fp64: the eight (or four) entries of a thread's 16-byte
//              piece in slab order, then block_sum_f64; one partial per block of 256 pieces; the stride's padding is not
//              counted.  dist = f16(sqrt(sum of the partials)) in one rounding (coevo_fc16_distance_finalize).
// A thread owns ONE 16-byte piece of the net (dqn16_pieces.hip.h, which also holds the noise of a piece: the float16 DeepQN
// Co-ES update of dqn16_es.hip regenerates it from there).  The roundings are f16_child / f16_diff of fc16_layout.hip.h, the
// distance loops those of f16_steps.hip.h.
#include <hip/hip_runtime.h>

#include "dqn16_pieces.hip.h"
#include "f16_steps.hip.h"

namespace coevo {

// grid (coevo_dqn16_perturb_blocks, n_children): dq16_perturb_dist_body (dqn16_pieces.hip.h) with the streamed fc1 block's noise
__global__ __launch_bounds__(256) void dqn16_perturb_dist_kernel(const uint32_t *parent_slab, const int32_t *parent_idx,
                                                                  uint32_t *child_slab, int child_first, int C, int n_actions,
                                                                  const float *sigma_dev, uint64_t seed,
                                                                  uint32_t stream_lo_first, uint32_t stream_hi, int flags,
                                                                  const int32_t *gen_dev, int gen_bias,
                                                                  const uint32_t *dist_ref, double *dist_partial)
{
    __shared__ double scratch[4];
    const Dq16PerturbArgs a{parent_slab, parent_idx, child_slab, child_first, C, n_actions, sigma_dev, seed, stream_lo_first,
                            stream_hi, flags, gen_dev, gen_bias, dist_ref, dist_partial};
    dq16_perturb_dist_body(a, scratch, [](int u, const DqnLayout &L, int C, float sigma, uint64_t seed, uint32_t slo, uint32_t shi,
                                          float (&noise)[8]) { dq16_fc1_piece_noise(u, L, C, sigma, seed, slo, shi, noise); });
}

// the same partials for nets that are already in a slab (generation 0, uploaded populations): grid (blocks, n)
__global__ __launch_bounds__(256) void dqn16_distance_kernel(const uint32_t *ref_net, const uint32_t *pop_slab, int C,
                                                              int n_actions, double *dist_partial)
{
    __shared__ double scratch[4];
    const int n = blockIdx.y, bx = blockIdx.x;
    const DqnLayout L = dqn16_layout(C, n_actions);
    const int u = bx * 256 + (int)threadIdx.x;
    double d2 = 0.0;
    if (u < dq16_pieces(L))
        d2 = dq16_piece_d2(reinterpret_cast<const uint4 *>(pop_slab + (int64_t)n * L.stride)[u],
                           reinterpret_cast<const uint4 *>(ref_net)[u], u, L);
    const double tot = block_sum_f64(d2, scratch);
    if (threadIdx.x == 0) dist_partial[(size_t)n * gridDim.x + bx] = tot;
}

}  // namespace coevo

using namespace coevo;

extern "C" int64_t coevo_dqn16_perturb_blocks(int C, int n_actions)
{
    return dqn_shape_ok(C, n_actions) ? (int64_t)dqn16_blocks(C, n_actions) : COEVO_ERR_ARG;
}

extern "C" int coevo_dqn16_perturb_dist(const void *parent_slab, const int32_t *parent_idx, void *child_slab, int child_first,
                                        int n_children, int C, int n_actions, const float *sigma_dev, uint64_t seed,
                                        uint32_t stream_lo_first, uint32_t stream_hi, int flags, const int32_t *gen_dev,
                                        int gen_bias, const void *dist_ref, double *dist_partial, void *stream)
{
    const int rc = dqn16_perturb_args(parent_slab, parent_idx, child_slab, child_first, n_children, C, n_actions, sigma_dev, flags,
                                      dist_ref, dist_partial);
    if (rc != COEVO_OK) return rc < 0 ? rc : COEVO_OK;
    const dim3 grid(dqn16_blocks(C, n_actions), (unsigned)n_children);
    hipLaunchKernelGGL(dqn16_perturb_dist_kernel, grid, dim3(256), 0, (hipStream_t)stream,
                       static_cast<const uint32_t *>(parent_slab), parent_idx, static_cast<uint32_t *>(child_slab), child_first,
                       C, n_actions, sigma_dev, seed, stream_lo_first, stream_hi, flags, gen_dev, gen_bias,
                       static_cast<const uint32_t *>(dist_ref), dist_partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_dqn16_distance(const void *ref_net, const void *pop_slab, int n, int C, int n_actions, double *dist_partial,
                                    void *stream)
{
    if (!ref_net || !pop_slab || !dist_partial || !dqn_shape_ok(C, n_actions) || n < 0 || n > 65535) return COEVO_ERR_ARG;
    if (!aligned16(ref_net) || !aligned16(pop_slab)) return COEVO_ERR_ARG;
    if (n == 0) return COEVO_OK;
    const dim3 grid(dqn16_blocks(C, n_actions), (unsigned)n);
    hipLaunchKernelGGL(dqn16_distance_kernel, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const uint32_t *>(ref_net),
                       static_cast<const uint32_t *>(pop_slab), C, n_actions, dist_partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
