// Float16 Co-GA breeding on the fp16 slab of fc16_layout.hip.h: offspring with their stale-agent distance fused in, the
// distance of nets already in a slab, its finalize with the fp16 rounding, net copies and the promotion.
//
// Replaces, for args.precision == "float16" (reference file:line): MPEAgent.clone + Agent.mutate (agent.py:25-29:
// half_param.data += torch.normal(0, sigma, size) - the sum in fp32, rounded once to half; LayerNorm affine stays fp32),
// np.linalg.norm(a16 - b16) of diversity_penalty on get_weights_ES() (utils/game_logic_functions.py:12-37) and the elite /
// Hall-of-Fame bookkeeping of genetic_algorithm.py:262-275.
//
// The float16 breeding contract (DESIGN.md "float16 nets"):
//   Linear weight or bias  child = f16(f32(parent) + noise), noise = sigma * eps(seed, stream, p) rounded to fp32 first,
//                          p the canonical flat parameters() index: the number the fp32 child of the same stream draws.
//                          Round to nearest even, past 65504 -> inf, fp16 subnormals kept.  A bias is an fp32 word that
//                          holds an fp16 value, before and after.
//   LayerNorm gamma / beta parent + noise in fp32, unrounded (left alone under COEVO_PERTURB_SKIP_LAYERNORM)
//   distance               per Linear entry d = f16(f32(a) - f32(b)); d * d accumulated in fp64: the eight (or four) entries
//                          of a thread's 16-byte piece in slab order, then block_sum_f64; one partial per 256-piece block.
//                          dist = f16(sqrt(sum of the partials)), stored as an fp32 word.
// A thread owns ONE 16-byte piece of the net (fc16_pieces.hip.h, which also holds the noise of a piece: the float16 Co-ES
// update of fc16_es.hip regenerates it from there).  The distance loops are those of f16_steps.hip.h (f16_diff of
// fc16_layout.hip.h).  The child sum of fc16_perturb_block is written out, not f16_child: its pin costs this kernel 2 - 3 % (it
// keeps the sums out of v_pk_add_f32; profiles/r21_fp16_steps_once.md), and the compiler does not fold this sum - the unit's
// disassembly holds no v_fma_mix* -, which tests/test_fp16_breeding_gpu.py decides word for word.
#include <hip/hip_runtime.h>

#include "f16_steps.hip.h"
#include "fc16_pieces.hip.h"
#include "promote_roles.hip.h"

namespace coevo {

// squared distance of piece u of net a to the same piece of net b: the piece's Linear entries in slab order
__device__ __forceinline__ double f16_piece_d2(const uint4 &a, const uint4 &b, int u, int D)
{
    if (u < f16_half_pieces(D)) return f16_d2_halves(a, b);
    return f16_d2_words(a, b, [=](int i) { return f16_tail_kind(4 * u + i, D) == 0; });
}

// one workgroup's 256 pieces of child c (block bx of nblocks); shared by the single- and the multi-role launch
__device__ __forceinline__ void fc16_perturb_block(const uint32_t *parent_slab, const int32_t *parent_idx, uint32_t *child_slab,
                                                   int child_first, int D, const float *sigma_dev, uint64_t seed,
                                                   uint32_t stream_lo_first, uint32_t stream_hi, int flags,
                                                   const int32_t *gen_dev, const uint32_t *dist_ref, double *dist_partial,
                                                   int c, int bx, int nblocks, double *scratch)
{
    if (gen_dev) stream_hi += 4u * (uint32_t)(*gen_dev);   // generation-indexed noise stream without a host argument
    const bool skip_layernorm = (flags & COEVO_PERTURB_SKIP_LAYERNORM) != 0;
    const uint32_t slo = stream_lo_first + (uint32_t)c;
    const int64_t stride = f16_stride(D);
    const int u = bx * 256 + (int)threadIdx.x;
    double d2 = 0.0;
    if (u < f16_pieces(D)) {
        const float sigma = *sigma_dev;
        const uint4 pv = reinterpret_cast<const uint4 *>(parent_slab + (int64_t)parent_idx[c] * stride)[u];
        uint4 ov;
        if (u < f16_half_pieces(D)) {
            float noise[8];
            f16_half_piece_noise(u, D, sigma, seed, slo, stream_hi, noise);
            _Float16 hin[8], hout[8];
            __builtin_memcpy(hin, &pv, sizeof(hin));
#pragma unroll
            for (int i = 0; i < 8; ++i) hout[i] = (_Float16)((float)hin[i] + noise[i]);   // the sum in fp32, rounded once to half
            __builtin_memcpy(&ov, hout, sizeof(hout));
        } else {
            const int w0 = 4 * u;
            float noise[4];
            f16_tail_piece_noise(u, D, sigma, seed, slo, stream_hi, noise);
            float in[4], out[4];
            __builtin_memcpy(in, &pv, sizeof(in));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kind = f16_tail_kind(w0 + i, D);
                const float v = in[i] + noise[i];
                out[i] = (kind == 0) ? f16r(v) : ((kind == 1 && !skip_layernorm) ? v : in[i]);
            }
            __builtin_memcpy(&ov, out, sizeof(out));
        }
        // a plain store: the rollout reads the child next
        reinterpret_cast<uint4 *>(child_slab + (int64_t)(child_first + c) * stride)[u] = ov;
        if (dist_partial) d2 = f16_piece_d2(ov, reinterpret_cast<const uint4 *>(dist_ref)[u], u, D);
    }
    if (dist_partial) {   // uniform over the workgroup
        const double tot = block_sum_f64(d2, scratch);
        if (threadIdx.x == 0) dist_partial[(size_t)c * nblocks + bx] = tot;
    }
}

// grid (f16_perturb_blocks(D), n_children): workgroup (bx, c) writes pieces 256 bx .. 256 bx + 255 of child c
__global__ __launch_bounds__(256) void fc16_perturb_dist_kernel(const uint32_t *parent_slab, const int32_t *parent_idx,
                                                                 uint32_t *child_slab, int child_first, int D,
                                                                 const float *sigma_dev, uint64_t seed,
                                                                 uint32_t stream_lo_first, uint32_t stream_hi, int flags,
                                                                 const int32_t *gen_dev, const uint32_t *dist_ref,
                                                                 double *dist_partial)
{
    __shared__ double scratch[4];
    fc16_perturb_block(parent_slab, parent_idx, child_slab, child_first, D, sigma_dev, seed, stream_lo_first, stream_hi, flags,
                       gen_dev, dist_ref, dist_partial, blockIdx.y, blockIdx.x, gridDim.x, scratch);
}

static_assert(sizeof(coevo_fc16_perturb_job) == 72, "layout mirrored by coevonet_amd/lib.py Perturb16Job");
struct Perturb16Jobs { coevo_fc16_perturb_job j[COEVO_MAX_JOBS]; };
// blockIdx.z = job (role); the grid covers the largest job, the surplus workgroups of the others leave at once.  A job's
// partials keep its OWN block count as their stride (f16_perturb_blocks(D): 70 or 69), not the grid's.
__global__ __launch_bounds__(256) void fc16_perturb_multi_kernel(Perturb16Jobs jobs, uint64_t seed, int flags,
                                                                  const int32_t *gen_dev)
{
    __shared__ double scratch[4];
    const coevo_fc16_perturb_job &jb = jobs.j[blockIdx.z];
    const int nblocks = f16_perturb_blocks(jb.D);
    if ((int)blockIdx.x >= nblocks || (int)blockIdx.y >= jb.n_children) return;   // workgroup-uniform, before any barrier
    fc16_perturb_block(static_cast<const uint32_t *>(jb.parent_slab), jb.parent_idx, static_cast<uint32_t *>(jb.child_slab),
                       jb.child_first, jb.D, jb.sigma_dev, seed, jb.stream_lo_first, jb.stream_hi, flags, gen_dev,
                       static_cast<const uint32_t *>(jb.dist_ref), jb.dist_partial, blockIdx.y, blockIdx.x, nblocks, scratch);
}

// the same partials for nets that are already in a slab (generation 0, uploaded populations): grid (blocks, n)
__global__ __launch_bounds__(256) void fc16_distance_kernel(const uint32_t *ref_net, const uint32_t *pop_slab, int D,
                                                             double *dist_partial)
{
    __shared__ double scratch[4];
    const int n = blockIdx.y, bx = blockIdx.x;
    const int u = bx * 256 + (int)threadIdx.x;
    double d2 = 0.0;
    if (u < f16_pieces(D))
        d2 = f16_piece_d2(reinterpret_cast<const uint4 *>(pop_slab + (int64_t)n * f16_stride(D))[u],
                          reinterpret_cast<const uint4 *>(ref_net)[u], u, D);
    const double tot = block_sum_f64(d2, scratch);
    if (threadIdx.x == 0) dist_partial[(size_t)n * gridDim.x + bx] = tot;
}

// dist[first + c] = f16(sqrt(sum_b partial[c][b])), dist_finalize_kernel's order; head: dist[first - 1] = *head
__global__ __launch_bounds__(64) void fc16_dist_finalize_kernel(const double *partial, int n_blocks, float *dist, int first,
                                                                 const float *head)
{
    const int c = blockIdx.x;
    const double v = wave_sum_partials(partial + (size_t)c * n_blocks, n_blocks);
    if (threadIdx.x == 0) {
        dist[first + c] = f16_of_f64(sqrt(v));
        if (c == 0 && head) dist[first - 1] = *head;
    }
}

// blockIdx.y = job: fc16_dist_finalize_kernel of each job in one launch (dist_finalize_multi_kernel with the fp16 rounding)
struct Finalize16Jobs { coevo_fc_finalize_job j[COEVO_MAX_JOBS]; };
__global__ __launch_bounds__(64) void fc16_dist_finalize_multi_kernel(Finalize16Jobs jobs)
{
    const coevo_fc_finalize_job &jb = jobs.j[blockIdx.y];
    const int c = blockIdx.x;
    if (c >= jb.n) return;
    const double v = wave_sum_partials(jb.dist_partial + (size_t)c * jb.n_blocks, jb.n_blocks);
    if (threadIdx.x == 0) {
        jb.dist[jb.first + c] = f16_of_f64(sqrt(v));
        if (c == 0 && jb.head) jb.dist[jb.first - 1] = *jb.head;
    }
}

// ---- elites -> elite buffer, HoF FIFO push, best -> pop[0] for up to three roles in one launch: ga_promote_kernel of
// offspring.hip on fp16 nets.  A thread owns one 16-byte piece of every net it touches and reads its piece of every source
// before the first store that could alias it; the pieces live in the frames of a compile-time recursion (loads on the way
// down, stores on the way back), so the in-place shift needs no second buffer and no runtime-indexed array.
struct Ga16PromoteArgs {
    coevo_ga16_promote_role role[3];
    int E, hof;
};

template <int I>
__device__ __forceinline__ void promote16_hof_shift(uint4 *hof, int64_t pitch, int n)
{
    if constexpr (I < PROMOTE_MAX_HOF) {
        const uint4 v = hof[(int64_t)(I < n ? I : n - 1) * pitch];
        promote16_hof_shift<I + 1>(hof, pitch, n);
        hof[(int64_t)(I < n ? I - 1 : n - 1) * pitch] = v;   // (a surplus level rewrites the last slot; the caller overwrites it)
    }
}

// elite[k] = pop[order[k]] for k < E (k descending on the way back); returns pop[order[0]]
template <int K>
__device__ __forceinline__ uint4 promote16_elites(const uint4 *pop, const int32_t *order, uint4 *elite, int64_t pitch, int E)
{
    if constexpr (K < PROMOTE_MAX_E) {
        const int kc = K < E ? K : E - 1;
        const uint4 v = pop[(int64_t)order[kc] * pitch];
        promote16_elites<K + 1>(pop, order, elite, pitch, E);
        elite[(int64_t)kc * pitch] = v;
        return v;
    } else {
        return make_uint4(0u, 0u, 0u, 0u);
    }
}

__global__ __launch_bounds__(256) void ga16_promote_kernel(Ga16PromoteArgs a)
{
    const unsigned y = blockIdx.y;
    const PromoteRole R = PROMOTE_ROLE(a, y);
    const int u = blockIdx.x * 256 + (int)threadIdx.x;
    if (u >= f16_pieces(R.D)) return;
    const int64_t pitch = f16_pieces(R.D);   // 16-byte pieces between consecutive nets
    uint4 *pop = static_cast<uint4 *>(R.pop) + u, *hof = static_cast<uint4 *>(R.hof) + u, *elite = static_cast<uint4 *>(R.elite) + u;
    const uint4 e0 = R.from_pop ? promote16_elites<0>(pop, R.order, elite, pitch, a.E) : elite[0];
    promote16_hof_shift<1>(hof, pitch, a.hof);
    hof[(int64_t)(a.hof - 1) * pitch] = e0;
    if (R.to_pop0) pop[0] = e0;
}

}  // namespace coevo

using namespace coevo;

extern "C" int64_t coevo_fc16_perturb_blocks(int D) { return fc_dim_ok(D) ? f16_perturb_blocks(D) : COEVO_ERR_ARG; }

// what one fp16 breeding job (the arguments of one coevo_fc16_perturb_dist call) must satisfy
static bool perturb16_job_ok(const coevo_fc16_perturb_job &j)
{
    if ((j.dist_ref == nullptr) != (j.dist_partial == nullptr)) return false;
    if (!j.parent_slab || !j.parent_idx || !j.child_slab || !j.sigma_dev || !fc_dim_ok(j.D)) return false;
    if (!aligned16(j.parent_slab) || !aligned16(j.child_slab) || !aligned16(j.dist_ref)) return false;
    return j.n_children >= 0 && j.child_first >= 0 && j.n_children <= 65535;
}

extern "C" int coevo_fc16_perturb_dist(const void *parent_slab, const int32_t *parent_idx, void *child_slab, int child_first,
                                       int n_children, int D, const float *sigma_dev, uint64_t seed,
                                       uint32_t stream_lo_first, uint32_t stream_hi, int flags, const int32_t *gen_dev,
                                       const void *dist_ref, double *dist_partial, void *stream)
{
    const coevo_fc16_perturb_job j{parent_slab, parent_idx, child_slab, sigma_dev, dist_ref, dist_partial,
                                   child_first, n_children, D, stream_lo_first, stream_hi, 0};
    if (!perturb16_job_ok(j) || (flags & ~COEVO_PERTURB_SKIP_LAYERNORM)) return COEVO_ERR_ARG;
    if (n_children == 0) return COEVO_OK;
    const dim3 grid((unsigned)f16_perturb_blocks(D), (unsigned)n_children);
    hipLaunchKernelGGL(fc16_perturb_dist_kernel, grid, dim3(256), 0, (hipStream_t)stream,
                       static_cast<const uint32_t *>(parent_slab), parent_idx, static_cast<uint32_t *>(child_slab),
                       child_first, D, sigma_dev, seed, stream_lo_first, stream_hi, flags, gen_dev,
                       static_cast<const uint32_t *>(dist_ref), dist_partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc16_perturb_dist_multi(const coevo_fc16_perturb_job *jobs, int n_jobs, uint64_t seed, int flags,
                                             const int32_t *gen_dev, void *stream)
{
    if (!jobs || n_jobs < 1 || n_jobs > COEVO_MAX_JOBS || (flags & ~COEVO_PERTURB_SKIP_LAYERNORM)) return COEVO_ERR_ARG;
    Perturb16Jobs pj{};
    unsigned gx = 0, gy = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const coevo_fc16_perturb_job &j = jobs[i];
        if (!perturb16_job_ok(j)) return COEVO_ERR_ARG;
        pj.j[i] = j;
        if (j.n_children == 0) continue;   // (an empty job does not widen the grid)
        const unsigned nb = (unsigned)f16_perturb_blocks(j.D);
        gx = nb > gx ? nb : gx;
        gy = (unsigned)j.n_children > gy ? (unsigned)j.n_children : gy;
    }
    if (gy == 0) return COEVO_OK;
    hipLaunchKernelGGL(fc16_perturb_multi_kernel, dim3(gx, gy, (unsigned)n_jobs), dim3(256), 0, (hipStream_t)stream, pj, seed,
                       flags, gen_dev);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc16_distance(const void *ref_net, const void *pop_slab, int n, int D, double *dist_partial, void *stream)
{
    if (!ref_net || !pop_slab || !dist_partial || !fc_dim_ok(D) || n < 0 || n > 65535) return COEVO_ERR_ARG;
    if (!aligned16(ref_net) || !aligned16(pop_slab)) return COEVO_ERR_ARG;
    if (n == 0) return COEVO_OK;
    const dim3 grid((unsigned)f16_perturb_blocks(D), (unsigned)n);
    hipLaunchKernelGGL(fc16_distance_kernel, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const uint32_t *>(ref_net),
                       static_cast<const uint32_t *>(pop_slab), D, dist_partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc16_distance_finalize(const double *dist_partial, int n_blocks, int n, float *dist, int first,
                                            const float *head, void *stream)
{
    if (!dist_partial || !dist || n_blocks <= 0 || n <= 0 || first < 0 || (head && first < 1)) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(fc16_dist_finalize_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, dist_partial, n_blocks, dist,
                       first, head);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc16_distance_finalize_multi(const coevo_fc_finalize_job *jobs, int n_jobs, void *stream)
{
    if (!jobs || n_jobs < 1 || n_jobs > COEVO_MAX_JOBS) return COEVO_ERR_ARG;
    Finalize16Jobs fj{};
    int nmax = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const coevo_fc_finalize_job &j = jobs[i];
        if (!j.dist_partial || !j.dist || j.n_blocks <= 0 || j.n < 0 || j.first < 0 || (j.head && j.first < 1)) return COEVO_ERR_ARG;
        fj.j[i] = j;
        nmax = j.n > nmax ? j.n : nmax;
    }
    if (nmax == 0) return COEVO_OK;
    hipLaunchKernelGGL(fc16_dist_finalize_multi_kernel, dim3((unsigned)nmax, (unsigned)n_jobs), dim3(64), 0, (hipStream_t)stream,
                       fj);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc16_gather(const void *src_slab, const int32_t *src_idx, void *dst_slab, int dst_first, int n, int D,
                                 void *stream)
{
    if (!src_slab || !src_idx || !dst_slab || !fc_dim_ok(D) || n < 0 || dst_first < 0 || n > 65535) return COEVO_ERR_ARG;
    if (!aligned16(src_slab) || !aligned16(dst_slab)) return COEVO_ERR_ARG;
    // whole 16-byte pieces of the stride: fc_gather_kernel's copy, f16_pieces(D) pieces per net
    return coevo_net_gather(static_cast<const float *>(src_slab), src_idx, static_cast<float *>(dst_slab), dst_first, n,
                            f16_stride(D), stream);
}

extern "C" int coevo_ga16_promote(const coevo_ga16_promote_role *roles, int n_roles, int E, int hof, void *stream)
{
    Ga16PromoteArgs a{};
    if (!promote_roles(a, roles, n_roles, E, hof, true)) return COEVO_ERR_ARG;
    int max_blocks = 0;
    for (int r = 0; r < n_roles; ++r) max_blocks = std::max(max_blocks, f16_perturb_blocks(roles[r].D));
    hipLaunchKernelGGL(ga16_promote_kernel, dim3((unsigned)max_blocks, (unsigned)n_roles), dim3(256), 0, (hipStream_t)stream, a);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
