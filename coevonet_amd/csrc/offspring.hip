// K3/K4/K5/K8 - building offspring weights on the device, plus slab <-> canonical-order packing.
//
// Replaces (reference file:line): MPEAgent.clone's state_dict copy (MPE/mpe_agent.py:24-28), Agent.mutate
// (agent.py:25-29: noise = torch.normal(0, sigma, size); param += noise for EVERY parameter, LayerNorm affine
// included), Agent.mutate_ES (agent.py:51-53: Linear weights/biases only) and compute_weight_update
// (evolutionary_strategy.py:120-148).
//
// Noise is counter-based so that no weight ever crosses PCIe: eps(seed, stream, p) for canonical flat index p is
// element p%4 of Philox4x32-7(counter = (p/4, stream_lo, stream_hi, 'coev'), key = seed) pushed through a
// Box-Muller transform whose log / sincos are fmaf-only polynomials (bit-identical with oracle/coevo_oracle.c).
// A child is one streaming pass: read parent (L2/Infinity-Cache resident elite), write child once.
#include "coevo_common.hip.h"
#include "dqn_common.hip.h"
#include "promote_roles.hip.h"
#include "philox.hip.h"

namespace coevo {

// Standard normals of the noise contract at slab positions.  Only fc1.weight is stored against the canonical order (W1t,
// transposed); everywhere else the four positions of a 16-byte piece are one canonical quad = one Philox block.  All index
// math is 32-bit (a net is < 2^18 floats).
//
// canonical quad of the W2q piece at slab position s0 (o_w2 <= s0 < o_b2, s0 % 4 == 0): W2q[jb][kq][l][0..3] are
// fc2.w[64 jb + l][4 kq .. 4 kq + 3]
__device__ __forceinline__ uint32_t w2_piece_quad(int32_t s0, int32_t o_w2)
{
    const int32_t t = s0 - o_w2;
    const int32_t l = (t >> 2) & 63, kq = (t >> 8) & 127, jb = t >> 15;
    return (uint32_t)((o_w2 + (jb * 64 + l) * H1 + kq * 4) >> 2);
}

// W1t slab position of canonical index p < D * 512: fc1.w[j][k] (p = j D + k) lies at W1t[k][j]
__device__ __forceinline__ int32_t w1t_slab_of_flat(uint32_t p, int D)
{
    const uint32_t j = (D == 8) ? (p >> 3) : (p / 10u);   // fc_dim_ok: D is 8 or 10
    return (int32_t)((p - j * (uint32_t)D) * H1 + j);
}

// the piece at s0 (s0 % 4 == 0, s0 < fc_stride(D)); z = 0 at padding words (s >= fc_params(D)), where a piece that is all
// padding costs no Philox block.  A W1t piece is four canonical quads of which it uses one normal each: whoever writes
// whole W1t rows goes through w1t_normals_to_lds instead (fc_perturb_block); the rebuild kernels' W1t pieces pass here.
__device__ inline void slab_quad_normals(uint64_t seed, uint32_t slo, uint32_t shi, int32_t s0, int D, float z[4])
{
    const int32_t o_b1 = (int32_t)fc_off_b1(D), o_w2 = (int32_t)fc_off_w2(D), o_b2 = (int32_t)fc_off_b2(D);
    const int32_t P = (int32_t)fc_params(D);
    if (s0 >= o_w2 && s0 < o_b2) {
        philox_normal4(seed, slo, shi, w2_piece_quad(s0, o_w2), z);
    } else if (s0 >= o_b1) {   // b1 g1 be1 | b2 g2 be2 W3 b3 | padding: slab position = canonical index
        if (s0 < P) {
            philox_normal4(seed, slo, shi, (uint32_t)s0 >> 2, z);
#pragma unroll
            for (int i = 1; i < 4; ++i) z[i] = (s0 + i < P) ? z[i] : 0.0f;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = 0.0f;
        }
    } else {
        const uint32_t k = (uint32_t)s0 >> 9, j = (uint32_t)s0 & (H1 - 1);   // W1t[k][j .. j + 3]
        // (one copy of the generator, four trips: unrolled, the four interleaved generators cost ga_promote_kernel a wave of
        // occupancy)
        z[0] = z[1] = z[2] = z[3] = 0.0f;
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const uint32_t p = (j + i) * (uint32_t)D + k;
            float zz[4];
            philox_normal4(seed, slo, shi, p >> 2, zz);
            const float v = zz[p & 3];
#pragma unroll
            for (int m = 0; m < 4; ++m) z[m] = (m == i) ? v : z[m];
        }
    }
}

constexpr int W1T_MAX_FLOATS = 10 * H1;   // W1t of the widest net (D = 10): 20 KiB of LDS
// The whole W1t region's normals by canonical quad: the workgroup's 256 threads run the D * 128 Philox blocks of fc1.weight
// once each (D / 2 per thread) and drop every normal at its slab position in `lds` ([D][512], the region's own layout).
// Ends with a barrier.
__device__ __forceinline__ void w1t_normals_to_lds(uint64_t seed, uint32_t slo, uint32_t shi, int D, float *lds)
{
    for (uint32_t q = threadIdx.x; q < (uint32_t)D * (H1 / 4); q += 256) {   // D * 128 is a multiple of 256
        float zz[4];
        philox_normal4(seed, slo, shi, q, zz);
#pragma unroll
        for (int i = 0; i < 4; ++i) lds[w1t_slab_of_flat(4 * q + i, D)] = zz[i];   // at D = 10 a quad straddles two rows j
    }
    __syncthreads();
}

// out = in + sigma * z (-: the odd partner of an antithetic pair) where not kept, stored at ch + s0; returns the piece's share
// of the squared distance to the reference net, 0 without one
__device__ __forceinline__ double perturb_apply_piece(float4 pv, const float z[4], const bool keep[4], const bool in_dist[4],
                                                      float sigma, bool negate, float *ch, const float *dist_ref, int32_t s0)
{
    const float in[4] = {pv.x, pv.y, pv.z, pv.w};
    float out[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float noise = sigma * z[i];  // rounded first, then added (agent.py:28-29)
        out[i] = keep[i] ? in[i] : in[i] + (negate ? -noise : noise);
    }
    *reinterpret_cast<float4 *>(ch + s0) = make_float4(out[0], out[1], out[2], out[3]);
    double d2 = 0.0;
    if (dist_ref) {  // fitness-sharing distance of the new child to a reference net, while it is in registers
        const float4 rv = *reinterpret_cast<const float4 *>(dist_ref + s0);
        const float ref[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (in_dist[i]) {
                const float d = out[i] - ref[i];
                d2 += (double)d * (double)d;
            }
        }
    }
    return d2;
}

// ---- the fp64 block reduction of the fused distance, in the vector ALU
template <int CTRL>
__device__ __forceinline__ double dpp_move_f64(double v)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <bool ROW32>
__device__ __forceinline__ double add_swap_f64(double v)   // v + v[lane ^ 16] (or ^ 32), as add_xor16 / add_xor32
{
    typedef unsigned u32x2_h __attribute__((ext_vector_type(2)));
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const u32x2_h l = ROW32 ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false)
                            : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const u32x2_h h = ROW32 ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false)
                            : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
}

// block_sum_f64 (same order of additions: lane xor 1, 2, 4, 8, 16, 32, then the four waves left to right) with the exchanges
// of the fp32 tree sums in coevo_common.hip.h - DPP and lane swaps in the vector ALU instead of twelve ds_bpermute - and ONE
// barrier: consecutive calls of a workgroup alternate between two scratch areas of four doubles (the barrier of call n + 1
// lies between the reads of call n and the writes of call n + 2).  fp64 addition commutes: the same bits.
__device__ __forceinline__ double breed_block_sum(double v, double *scratch)
{
    v = v + dpp_move_f64<0xB1>(v);    // quad_perm [1,0,3,2]
    v = v + dpp_move_f64<0x4E>(v);    // quad_perm [2,3,0,1]
    v = v + dpp_move_f64<0x141>(v);   // row_half_mirror
    v = v + dpp_move_f64<0x140>(v);   // row_mirror
    v = add_swap_f64<false>(v);
    v = add_swap_f64<true>(v);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

// how many of the blocks that lie in W2 as a whole one workgroup takes, straight-line: the prologue and the generator's
// constants are paid once, the generators interleave.  2 and 4 measured alike (profiles/r24_breeding_regions.md)
#ifndef COEVO_BREED_U
#define COEVO_BREED_U 2
#endif

// LDS of a breeding workgroup: the W1t region's normals; its first 64 bytes double as the block reductions' scratch
// (two areas of four doubles)
struct alignas(16) PerturbLds { float z[W1T_MAX_FLOATS]; };

// one workgroup's 1024 slab positions of child c (block bx of nblocks); shared by the single- and the multi-role launch.
// Workgroup 0 of a child owns the whole W1t region (blocks 0 .. D/2 - 1, one after the other: same thread per position,
// one block reduction per block); the workgroups of blocks 1 .. D/2 - 1 leave at once.  Likewise every COEVO_BREED_U-th
// workgroup of the blocks that lie in W2 as a whole takes COEVO_BREED_U of them and the ones between leave at once.  The grid
// and dist_partial[(child, block)] stay what coevo_fc_perturb_blocks says.
__device__ __forceinline__ void fc_perturb_block(const float *parent_slab, const int32_t *parent_idx, float *child_slab,
                                                 int child_first, int D, const float *sigma_dev, uint64_t seed,
                                                 uint32_t stream_lo_first, uint32_t stream_hi, int skip_layernorm,
                                                 const int32_t *gen_dev, const float *dist_ref, double *dist_partial,
                                                 int c, int bx, int nblocks, PerturbLds &lds)
{
    const int w1t_blocks = D / 2;   // D * 512 / 1024
    if (bx > 0 && bx < w1t_blocks) return;   // workgroup-uniform
    if (gen_dev) stream_hi += 4u * (uint32_t)(*gen_dev);  // generation-indexed noise stream without a host argument
    // flags: bit 0 = leave LayerNorm affine untouched (ES), bit 1 = antithetic pairs (extension mode): individuals 2m and
    // 2m+1 share noise stream m, the odd one takes -eps
    const bool antithetic = (skip_layernorm & 2) != 0;
    skip_layernorm &= 1;
    const uint32_t ind = stream_lo_first + (uint32_t)c;
    const uint32_t slo = antithetic ? (ind >> 1) : ind;
    const bool negate = antithetic && (ind & 1u);
    const int64_t stride = fc_stride(D);
    const float sigma = *sigma_dev;
    const float *par = parent_slab + (int64_t)parent_idx[c] * stride;
    float *ch = child_slab + (int64_t)(child_first + c) * stride;
    double *scratch = reinterpret_cast<double *>(lds.z);
    if (bx == 0) {
        w1t_normals_to_lds(seed, slo, stream_hi, D, lds.z);
        const float4 *zl = reinterpret_cast<const float4 *>(lds.z);
        float4 zv = zl[threadIdx.x];
        __syncthreads();   // block 0's normals are in registers: its first words are the reductions' scratch from here on
        const bool keep[4] = {false, false, false, false}, in_dist[4] = {true, true, true, true};   // W1t: no LayerNorm, no padding
        for (int b = 0; b < w1t_blocks; ++b) {
            const int32_t s0 = (b * 256 + (int32_t)threadIdx.x) * 4;
            const float4 pv = *reinterpret_cast<const float4 *>(par + s0);
            const float z[4] = {zv.x, zv.y, zv.z, zv.w};
            const double d2 = perturb_apply_piece(pv, z, keep, in_dist, sigma, negate, ch, dist_ref, s0);
            if (b + 1 < w1t_blocks) zv = zl[(b + 1) * 256 + threadIdx.x];
            if (dist_partial) {  // workgroup-uniform
                const double tot = breed_block_sum(d2, scratch + 4 * (b & 1));
                if (threadIdx.x == 0) dist_partial[(size_t)c * nblocks + b] = tot;
            }
        }
        return;
    }
#if COEVO_BREED_U > 1
    {
        const int32_t o_w2 = (int32_t)fc_off_w2(D), o_b2 = (int32_t)fc_off_b2(D);
        const int w2_first = (o_w2 + 1023) >> 10, w2_end = o_b2 >> 10;
        if (bx >= w2_first && bx < w2_end) {
            if ((bx - w2_first) % COEVO_BREED_U) return;   // workgroup-uniform
            const int run = min(COEVO_BREED_U, w2_end - bx);
            const bool keep[4] = {false, false, false, false}, in_dist[4] = {true, true, true, true};
            double d2u[COEVO_BREED_U];
#pragma unroll
            for (int u = 0; u < COEVO_BREED_U; ++u) {
                d2u[u] = 0.0;
                if (u < run) {
                    const int32_t s0 = ((bx + u) * 256 + (int32_t)threadIdx.x) * 4;
                    const float4 pv = *reinterpret_cast<const float4 *>(par + s0);
                    float z[4];
                    philox_normal4(seed, slo, stream_hi, w2_piece_quad(s0, o_w2), z);
                    d2u[u] = perturb_apply_piece(pv, z, keep, in_dist, sigma, negate, ch, dist_ref, s0);
                }
            }
            if (dist_partial) {
#pragma unroll
                for (int u = 0; u < COEVO_BREED_U; ++u) {
                    if (u < run) {
                        const double tot = breed_block_sum(d2u[u], scratch + 4 * (u & 1));
                        if (threadIdx.x == 0) dist_partial[(size_t)c * nblocks + bx + u] = tot;
                    }
                }
            }
            return;
        }
    }
#endif
    const int32_t s0 = (bx * 256 + (int32_t)threadIdx.x) * 4;
    double d2 = 0.0;
    if (s0 < (int32_t)stride) {
        const float4 pv = *reinterpret_cast<const float4 *>(par + s0);
        float z[4];
        bool keep[4], in_dist[4];
        const int32_t o_w2 = (int32_t)fc_off_w2(D), o_b2 = (int32_t)fc_off_b2(D);
        if (s0 >= o_w2 && s0 < o_b2) {
            // fc2 block (93.8 % of a net): one Philox block, never LayerNorm, never padding
            philox_normal4(seed, slo, stream_hi, w2_piece_quad(s0, o_w2), z);
#pragma unroll
            for (int i = 0; i < 4; ++i) { keep[i] = false; in_dist[i] = true; }
        } else {
            // b1 g1 be1 | b2 g2 be2 W3 b3 | padding: every region edge but the last parameter is a multiple of 4, so a piece
            // is LayerNorm or not as a whole
            slab_quad_normals(seed, slo, stream_hi, s0, D, z);
            const int32_t g1 = (int32_t)fc_off_g1(D), g2 = (int32_t)fc_off_g2(D), P = (int32_t)fc_params(D);
            const bool ln = (s0 >= g1 && s0 < g1 + 2 * H1) || (s0 >= g2 && s0 < g2 + 2 * H2);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool pad = s0 + i >= P;
                keep[i] = pad || (skip_layernorm && ln);
                in_dist[i] = !pad && !ln;
            }
        }
        d2 = perturb_apply_piece(pv, z, keep, in_dist, sigma, negate, ch, dist_ref, s0);
    }
    if (dist_partial) {  // wave-uniform
        const double tot = breed_block_sum(d2, scratch);
        if (threadIdx.x == 0) dist_partial[(size_t)c * nblocks + bx] = tot;
    }
}

__global__ __launch_bounds__(256) void fc_perturb_kernel(const float *parent_slab, const int32_t *parent_idx,
                                                          float *child_slab, int child_first, int D,
                                                          const float *sigma_dev, uint64_t seed,
                                                          uint32_t stream_lo_first, uint32_t stream_hi,
                                                          int skip_layernorm, const int32_t *gen_dev,
                                                          const float *dist_ref, double *dist_partial)
{
    __shared__ PerturbLds lds;
    fc_perturb_block(parent_slab, parent_idx, child_slab, child_first, D, sigma_dev, seed, stream_lo_first, stream_hi,
                     skip_layernorm, gen_dev, dist_ref, dist_partial, blockIdx.y, blockIdx.x, gridDim.x, lds);
}

static_assert(sizeof(coevo_fc_perturb_job) == 72, "layout mirrored by coevonet_amd/lib.py PerturbJob");
struct PerturbJobs { coevo_fc_perturb_job j[COEVO_MAX_JOBS]; };
// blockIdx.z = job (role); the grid covers the largest job, the surplus workgroups of the others leave at once
__global__ __launch_bounds__(256) void fc_perturb_multi_kernel(PerturbJobs jobs, uint64_t seed, int skip_layernorm,
                                                                const int32_t *gen_dev)
{
    __shared__ PerturbLds lds;
    const coevo_fc_perturb_job &jb = jobs.j[blockIdx.z];
    const int nblocks = (int)quad_blocks(fc_stride(jb.D));
    if ((int)blockIdx.x >= nblocks || (int)blockIdx.y >= jb.n_children) return;   // workgroup-uniform
    fc_perturb_block(jb.parent_slab, jb.parent_idx, jb.child_slab, jb.child_first, jb.D, jb.sigma_dev, seed,
                     jb.stream_lo_first, jb.stream_hi, skip_layernorm, gen_dev, jb.dist_ref, jb.dist_partial, blockIdx.y,
                     blockIdx.x, nblocks, lds);
}

// New elites without gathering them from whichever GPU evaluated them: elite e of this generation is individual
// id = order[e] of the population that was bred from `elite_prev` one generation ago, so any rank can rebuild it:
//   id == 0      -> last generation's best, elite_prev[0], unchanged
//   id >= 1      -> elite_prev[(id-1) % E] + sigma_prev * eps(seed, stream (id-1, stream_hi_prev))   (same bits as the
//                   child the owning rank materialised: same kernel arithmetic, same counters)
__global__ __launch_bounds__(256) void fc_rebuild_elites_kernel(const float *elite_prev, const int32_t *order,
                                                                 float *elite_new, int E, int D,
                                                                 const float *sigma_prev_dev, uint64_t seed,
                                                                 uint32_t stream_hi_prev, const int32_t *gen_dev)
{
    if (gen_dev) stream_hi_prev += 4u * (uint32_t)(*gen_dev - 1);
    const int e = blockIdx.y;
    const int64_t stride = fc_stride(D), P = fc_params(D);
    const int64_t s0 = quad_first(blockIdx.x);
    if (s0 >= stride) return;
    const int id = order[e];
    float *dst = elite_new + (int64_t)e * stride;
    if (id == 0) {
        *reinterpret_cast<float4 *>(dst + s0) = *reinterpret_cast<const float4 *>(elite_prev + s0);
        return;
    }
    const int c = id - 1;
    const float sigma = *sigma_prev_dev;
    const float4 pv = *reinterpret_cast<const float4 *>(elite_prev + (int64_t)(c % E) * stride + s0);
    float z[4];
    slab_quad_normals(seed, (uint32_t)c, stream_hi_prev, (int32_t)s0, D, z);
    const float in[4] = {pv.x, pv.y, pv.z, pv.w};
    float out[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = (s0 + i >= P) ? in[i] : in[i] + sigma * z[i];
    *reinterpret_cast<float4 *>(dst + s0) = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(256) void fc_gather_kernel(const float *src_slab, const int32_t *src_idx,
                                                         float *dst_slab, int dst_first, int64_t stride)
{
    const int c = blockIdx.y;
    const int64_t s0 = quad_first(blockIdx.x);
    if (s0 >= stride) return;
    const float4 v = *reinterpret_cast<const float4 *>(src_slab + (int64_t)src_idx[c] * stride + s0);
    *reinterpret_cast<float4 *>(dst_slab + (int64_t)(dst_first + c) * stride + s0) = v;
}

// ---- elites -> elite buffer, HoF FIFO push, best -> pop[0] for up to three roles in ONE launch (instead of five net
// copies per role).  A thread owns one 16-byte piece of every net it touches: it reads its piece of all sources first,
// so the in-place HoF shift and a best individual that already sits in pop[0] need no second buffer.  What this launch
// shares with ga16_promote_kernel (fc16_offspring.hip) is in promote_roles.hip.h.
struct GaPromoteArgs {
    coevo_ga_promote_role role[3];
    int E, hof;
    // rebuild mode (coevo_ga_promote_rebuild): the new elites are not in `elite` yet - elite[k] is individual order[k] of the
    // generation just evaluated, i.e. the unchanged best (id 0 = old elite 0) or child c = id - 1 = old elite[c % E] +
    // sigma * noise(c), regenerated here from the OLD elites in place
    const float *sigma;          // [3] device: what that generation's children were bred with; NULL: not rebuild mode
    const int32_t *gen_dev;      // device generation counter g (the children were bred with streams of g - 1), or NULL
    uint64_t seed;
    uint32_t stream_hi_prev;     // + role index (+ 4 (g - 1) with gen_dev)
    int32_t *tick;               // NULL, or the generation counter this launch increments (nothing in it reads the counter
                                 // after the first instructions of its blocks: see ga_promote_kernel)
};

// A thread's 16-byte pieces are held in the frames of a compile-time recursion - every load on the way down, every store
// on the way back - not in arrays: as float4 e[8], h[16] filled by unrolled loops the compiler left both in scratch
// (400 bytes per lane).  Loads take clamped indices and stores are unconditional; a surplus level (index >= count)
// rewrites the last slot with the value it holds anyway or that the caller overwrites next (same thread, same address,
// program order).
template <int I>
__device__ __forceinline__ void promote_hof_shift(float *hof, int64_t stride, int64_t s0, int n)
{
    if constexpr (I < PROMOTE_MAX_HOF) {
        const float4 v = *reinterpret_cast<const float4 *>(hof + (int64_t)(I < n ? I : n - 1) * stride + s0);
        promote_hof_shift<I + 1>(hof, stride, s0, n);
        *reinterpret_cast<float4 *>(hof + (int64_t)(I < n ? I - 1 : n - 1) * stride + s0) = v;
    }
}

// elite[k] = src[idx(k)] for k < E (k descending on the way back); returns src[idx(0)]
template <int K>
__device__ __forceinline__ float4 promote_elites(const float *src, const int32_t *order, float *elite, int64_t stride, int64_t s0,
                                                 int E)
{
    if constexpr (K < PROMOTE_MAX_E) {
        const int kc = K < E ? K : E - 1;
        const float4 v = *reinterpret_cast<const float4 *>(src + (int64_t)(order ? order[kc] : kc) * stride + s0);
        promote_elites<K + 1>(src, order, elite, stride, s0, E);
        *reinterpret_cast<float4 *>(elite + (int64_t)kc * stride + s0) = v;
        return v;
    } else {
        return make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// rebuild mode: every OLD elite piece a new elite needs is loaded on the way down, the new pieces are stored on the way back
// (each slab position depends only on the old elites' values at the same position: in place, no second elite buffer)
template <int K>
__device__ __forceinline__ float4 promote_rebuild(float *elite, const int32_t *order, int64_t stride, int64_t s0, int E, int D,
                                                  float sigma, uint64_t seed, uint32_t shi)
{
    if constexpr (K < PROMOTE_MAX_E) {
        const int kc = K < E ? K : E - 1;
        const int id = order[kc];
        const int c = id > 0 ? id - 1 : 0;
        const float4 pv = *reinterpret_cast<const float4 *>(elite + (int64_t)(id > 0 ? c % E : 0) * stride + s0);
        promote_rebuild<K + 1>(elite, order, stride, s0, E, D, sigma, seed, shi);
        float4 nv = pv;
        if (id > 0 && K < E) {   // (a surplus level re-stores slot E - 1 with the piece it loaded; level E - 1 overwrites it after)
            const int64_t P = fc_params(D);
            float z[4];
            slab_quad_normals(seed, (uint32_t)c, shi, (int32_t)s0, D, z);
            const float in[4] = {pv.x, pv.y, pv.z, pv.w};
            float out[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) out[i] = (s0 + i >= P) ? in[i] : in[i] + sigma * z[i];   // as fc_rebuild_elites_kernel
            nv = make_float4(out[0], out[1], out[2], out[3]);
        }
        *reinterpret_cast<float4 *>(elite + (int64_t)kc * stride + s0) = nv;
        return nv;
    } else {
        return make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__global__ __launch_bounds__(256) void ga_promote_kernel(GaPromoteArgs a)
{
    const unsigned y = blockIdx.y;
    const PromoteRole R = PROMOTE_ROLE(a, y);
    float *pop = static_cast<float *>(R.pop), *hof = static_cast<float *>(R.hof), *elite = static_cast<float *>(R.elite);
    const int64_t stride = fc_stride(R.D);
    // (written out, not quad_first: through the function this kernel's instructions and SGPR count move)
    const int64_t s0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (s0 >= stride) return;
    // every source piece is read before the first store that could alias it (a best individual that already sits in
    // pop[0], the in-place HoF shift)
    float4 e0;
    if (a.sigma && !R.from_pop) {
        uint32_t shi = a.stream_hi_prev + y;
        if (a.gen_dev) shi += 4u * (uint32_t)(*a.gen_dev - 1);
        e0 = promote_rebuild<0>(elite, R.order, stride, s0, a.E, R.D, a.sigma[y], a.seed, shi);
    } else {
        e0 = R.from_pop ? promote_elites<0>(pop, R.order, elite, stride, s0, a.E)
                        : *reinterpret_cast<const float4 *>(elite + s0);
    }
    promote_hof_shift<1>(hof, stride, s0, a.hof);
    *reinterpret_cast<float4 *>(hof + (int64_t)(a.hof - 1) * stride + s0) = e0;
    if (R.to_pop0) *reinterpret_cast<float4 *>(pop + s0) = e0;
    // the generation counter's tick (coevo_ga_promote_tick: only without gen_dev - no block of this launch reads the counter)
    if (a.tick && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.tick += 1;
}

// ---- tile-major twins of W2 (COEVO_TASK_TILED: what the lean shared-opponent body feeds its matrix instructions as loaded).
// Inside every group of 64 pieces (output block w, k-quad q) twin piece l = 16 lg + lc, element T is the net's piece
// 16 T + lc, element lg.  t0: the first float of the thread's OWN twin piece inside the W2 block; w2: the net's W2 block.
constexpr int64_t W2_FLOATS = (int64_t)H1 * H2;
__device__ __forceinline__ float4 w2_twin_piece(const float *w2, int64_t t0)
{
    const int64_t group = t0 & ~(int64_t)255;
    const int l = (int)(t0 >> 2) & 63, lc = l & 15, lg = l >> 4;
    const float *p = w2 + group + 4 * lc + lg;
    return make_float4(p[0], p[64], p[128], p[192]);
}

__global__ __launch_bounds__(256) void fc_w2_tile_major_kernel(const float *src, float *dst, int64_t stride, int64_t o_w2)
{
    const int64_t t0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;   // (the grid covers the W2 block exactly)
    *reinterpret_cast<float4 *>(dst + (int64_t)blockIdx.y * W2_FLOATS + t0) = w2_twin_piece(src + (int64_t)blockIdx.y * stride + o_w2, t0);
}

// twin slot I -> I - 1 for I < n, every load before the first store as in promote_hof_shift - but no surplus store: the last
// slot belongs to the caller alone
template <int I>
__device__ __forceinline__ void promote_twin_shift(float *twin, int64_t t0, int n)
{
    if constexpr (I < PROMOTE_MAX_HOF) {
        const float4 v = *reinterpret_cast<const float4 *>(twin + (int64_t)(I < n ? I : n - 1) * W2_FLOATS + t0);
        promote_twin_shift<I + 1>(twin, t0, n);
        if (I < n) *reinterpret_cast<float4 *>(twin + (int64_t)(I - 1) * W2_FLOATS + t0) = v;
    }
}

// ga_promote_kernel without the rebuild mode + the twins of role y's Hall of Fame, a.twins [role][hof][W2_FLOATS]: a thread whose
// piece lies in W2 owns the same piece of every twin slot - it shifts them with the FIFO and gathers the new member's from the
// best's net.  (That net is pop[order[0]] or elite[0]; the only store of this launch that can alias it is pop[0] = itself.)
__global__ __launch_bounds__(256) void ga_promote_tiled_kernel(GaPromoteArgs a, float *twins)
{
    const unsigned y = blockIdx.y;
    const PromoteRole R = PROMOTE_ROLE(a, y);
    float *pop = static_cast<float *>(R.pop), *hof = static_cast<float *>(R.hof), *elite = static_cast<float *>(R.elite);
    const int64_t stride = fc_stride(R.D);
    const int64_t s0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (s0 >= stride) return;
    const int64_t t0 = s0 - fc_off_w2(R.D);
    const bool in_w2 = t0 >= 0 && t0 < W2_FLOATS;
    float *twin = twins + (int64_t)y * a.hof * W2_FLOATS;
    float4 tw = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in_w2) {
        const float *best = R.from_pop ? pop + (int64_t)R.order[0] * stride : elite;
        tw = w2_twin_piece(best + fc_off_w2(R.D), t0);
        promote_twin_shift<1>(twin, t0, a.hof);
    }
    const float4 e0 = R.from_pop ? promote_elites<0>(pop, R.order, elite, stride, s0, a.E)
                                 : *reinterpret_cast<const float4 *>(elite + s0);
    promote_hof_shift<1>(hof, stride, s0, a.hof);
    *reinterpret_cast<float4 *>(hof + (int64_t)(a.hof - 1) * stride + s0) = e0;
    if (R.to_pop0) *reinterpret_cast<float4 *>(pop + s0) = e0;
    if (in_w2) *reinterpret_cast<float4 *>(twin + (int64_t)(a.hof - 1) * W2_FLOATS + t0) = tw;
    if (a.tick && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.tick += 1;
}

// sum over the individuals i = lo .. hi - 1, ascending, of fitness[i] * (pert_i - theta) at the thread's four slab positions,
// one fmaf per term starting from 0; pp = the thread's quad of individual 0, the nets `stride` floats apart.
// The perturbed nets are read exactly once: non-temporal, and 16 rows in flight per lane (only stride/1024 = 137
// workgroups exist per chunk - the sum over i is sequential by definition - so the memory-level parallelism comes from depth)
__device__ __forceinline__ float4 es_chunk_sum(float4 tv, const float *pp, int64_t stride, const float *fitness, int lo, int hi)
{
    const float th[4] = {tv.x, tv.y, tv.z, tv.w};
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    typedef float f32x4_nt __attribute__((ext_vector_type(4)));
    constexpr int UE = 16;
    int i = lo;
    for (; i + UE <= hi; i += UE) {
        float4 pv[UE];
#pragma unroll
        for (int u = 0; u < UE; ++u) {
            const f32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt *>(pp + (int64_t)(i + u) * stride));
            pv[u] = make_float4(v[0], v[1], v[2], v[3]);
        }
#pragma unroll
        for (int u = 0; u < UE; ++u) {
            const float f = fitness[i + u];
            acc[0] = __builtin_fmaf(f, pv[u].x - th[0], acc[0]);
            acc[1] = __builtin_fmaf(f, pv[u].y - th[1], acc[1]);
            acc[2] = __builtin_fmaf(f, pv[u].z - th[2], acc[2]);
            acc[3] = __builtin_fmaf(f, pv[u].w - th[3], acc[3]);
        }
    }
    for (; i < hi; ++i) {
        const float4 pv = *reinterpret_cast<const float4 *>(pp + (int64_t)i * stride);
        const float f = fitness[i];
        acc[0] = __builtin_fmaf(f, pv.x - th[0], acc[0]);
        acc[1] = __builtin_fmaf(f, pv.y - th[1], acc[1]);
        acc[2] = __builtin_fmaf(f, pv.z - th[2], acc[2]);
        acc[3] = __builtin_fmaf(f, pv.w - th[3], acc[3]);
    }
    return make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// the update's last step: theta + scale * sum at the four slab positions from s0, except where skip(s) keeps theta's word
template <class Skip>
__device__ __forceinline__ float4 es_step_quad(float4 tv, float4 av, float scale, int64_t s0, const Skip &skip)
{
    const float th[4] = {tv.x, tv.y, tv.z, tv.w}, acc[4] = {av.x, av.y, av.z, av.w};
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = skip(s0 + c) ? th[c] : th[c] + scale * acc[c];
    return make_float4(out[0], out[1], out[2], out[3]);
}

// theta[p] += lr/(n*sigma) * sum_i fitness[i] * (pert_i[p] - theta[p]), i ascending, one fmaf per term.
// The perturbation is read back from the materialised perturbed nets (one coalesced streaming pass over n*4P bytes)
// instead of being regenerated: 0.3 ms instead of 2 ms per role at n = 1000.  LayerNorm entries are never perturbed
// (their difference is exactly 0) and are skipped.
__global__ __launch_bounds__(256) void es_update_kernel(float *theta, const float *pert_slab, int D,
                                                         const float *fitness, int n, const float *sigma_dev, float lr)
{
    const int64_t stride = fc_stride(D), P = fc_params(D);
    const int64_t s0 = quad_first(blockIdx.x);
    if (s0 >= stride) return;
    const float sigma = *sigma_dev;
    const float scale = lr / ((float)n * sigma);
    const float4 tv = *reinterpret_cast<const float4 *>(theta + s0);
    const float4 av = es_chunk_sum(tv, pert_slab + s0, stride, fitness, 0, n);
    *reinterpret_cast<float4 *>(theta + s0) =
        es_step_quad(tv, av, scale, s0, [=](int64_t s) { return s >= P || fc_slab_is_layernorm(s, D); });
}

// K5 in two steps.  Step 1: partial[c][p] = sum over the individuals i of chunk c (global chunk gc = chunk_first + c
// covers [gc*n/C, (gc+1)*n/C)), i ascending, of fitness[i] * (pert_i[p] - theta[p]), one fmaf per term starting from
// 0.  grid (stride/1024, n_chunks): C times the workgroups of the sequential form (137 of them fill half the chip), and
// a population shard computes exactly its own chunks.  Step 2 (es_apply_kernel): theta += scale * (((p_0 + p_1) + p_2)
// + ...).  chunks_total = 1 is the sequential sum of es_update_kernel, bit for bit.
__global__ __launch_bounds__(256) void es_partial_kernel(const float *theta, const float *pert_slab, int ind_first,
                                                          int64_t stride, const float *fitness_all, int n_total,
                                                          int chunks_total, int chunk_first, float *partial)
{
    const int64_t s0 = quad_first(blockIdx.x);
    if (s0 >= stride) return;
    const int gc = chunk_first + blockIdx.y;
    const int i_lo = (int)((int64_t)gc * n_total / chunks_total), i_hi = (int)((int64_t)(gc + 1) * n_total / chunks_total);
    const float4 tv = *reinterpret_cast<const float4 *>(theta + s0);
    const float *pp = pert_slab + s0 - (int64_t)ind_first * stride;  // indexed by the GLOBAL individual
    *reinterpret_cast<float4 *>(partial + (int64_t)blockIdx.y * stride + s0) = es_chunk_sum(tv, pp, stride, fitness_all, i_lo, i_hi);
}

// partial of global chunk c lives at partials + (c / chunks_per_block) * block_stride + (c % chunks_per_block) * stride
// (one block per rank after the all-gather; a single block on one GPU)
// which slab positions an ES update leaves alone: padding (>= total) and up to three normalisation-affine ranges
struct SlabSkip {
    int64_t total, a0, b0, a1, b1, a2, b2;
    __host__ __device__ bool operator()(int64_t s) const
    {
        return s >= total || (s >= a0 && s < b0) || (s >= a1 && s < b1) || (s >= a2 && s < b2);
    }
};

__global__ __launch_bounds__(256) void es_apply_kernel(float *theta, const float *partials, int chunks_total,
                                                        int chunks_per_block, int64_t block_stride, int64_t stride,
                                                        SlabSkip skip, int n_total, const float *sigma_dev, float lr)
{
    const int64_t s0 = quad_first(blockIdx.x);
    if (s0 >= stride) return;
    const float sigma = *sigma_dev;
    const float scale = lr / ((float)n_total * sigma);
    float4 tot = *reinterpret_cast<const float4 *>(partials + s0);
    for (int c = 1; c < chunks_total; ++c) {
        const float4 v = *reinterpret_cast<const float4 *>(partials + (int64_t)(c / chunks_per_block) * block_stride +
                                                           (int64_t)(c % chunks_per_block) * stride + s0);
        tot.x = tot.x + v.x; tot.y = tot.y + v.y; tot.z = tot.z + v.z; tot.w = tot.w + v.w;
    }
    const float4 tv = *reinterpret_cast<const float4 *>(theta + s0);
    *reinterpret_cast<float4 *>(theta + s0) = es_step_quad(tv, tot, scale, s0, skip);
}

__global__ __launch_bounds__(256) void fc_pack_kernel(const float *flat, float *slab, int D, bool to_slab)
{
    const int net = blockIdx.y;
    const int64_t stride = fc_stride(D), P = fc_params(D);
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= stride) return;
    if (to_slab) {
        slab[(int64_t)net * stride + s] = (s < P) ? flat[(int64_t)net * P + fc_slab_to_flat(s, D)] : 0.0f;
    } else if (s < P) {
        const_cast<float *>(flat)[(int64_t)net * P + fc_slab_to_flat(s, D)] = slab[(int64_t)net * stride + s];
    }
}

}  // namespace coevo

using namespace coevo;

extern "C" int64_t coevo_fc_param_count(int D) { return fc_dim_ok(D) ? fc_params(D) : COEVO_ERR_ARG; }
extern "C" int64_t coevo_fc_slab_stride(int D) { return fc_dim_ok(D) ? fc_stride(D) : COEVO_ERR_ARG; }

extern "C" int coevo_fc_pack(const float *flat, float *slab, int n, int D, void *stream)
{
    if (!flat || !slab || n <= 0 || !fc_dim_ok(D)) return COEVO_ERR_ARG;
    const dim3 grid((unsigned)((fc_stride(D) + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(fc_pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, flat, slab, D, true);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc_unpack(const float *slab, float *flat, int n, int D, void *stream)
{
    if (!flat || !slab || n <= 0 || !fc_dim_ok(D)) return COEVO_ERR_ARG;
    const dim3 grid((unsigned)((fc_stride(D) + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(fc_pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float *)flat,
                       const_cast<float *>(slab), D, false);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int64_t coevo_fc_perturb_blocks(int D) { return fc_dim_ok(D) ? (int64_t)quad_blocks(fc_stride(D)) : COEVO_ERR_ARG; }

// what one breeding job (the arguments of one coevo_fc_perturb_dist call) must satisfy
static bool perturb_job_ok(const coevo_fc_perturb_job &j)
{
    if ((j.dist_ref == nullptr) != (j.dist_partial == nullptr)) return false;
    if (!j.parent_slab || !j.parent_idx || !j.child_slab || !j.sigma_dev || !fc_dim_ok(j.D)) return false;
    return j.n_children >= 0 && j.child_first >= 0 && j.n_children <= 65535;
}

extern "C" int coevo_fc_perturb_dist(const float *parent_slab, const int32_t *parent_idx, float *child_slab,
                                     int child_first, int n_children, int D, const float *sigma_dev, uint64_t seed,
                                     uint32_t stream_lo_first, uint32_t stream_hi, int skip_layernorm,
                                     const int32_t *gen_dev, const float *dist_ref, double *dist_partial, void *stream)
{
    const coevo_fc_perturb_job j{parent_slab, parent_idx, child_slab, sigma_dev, dist_ref, dist_partial,
                                 child_first, n_children, D, stream_lo_first, stream_hi, 0};
    if (!perturb_job_ok(j) || skip_layernorm < 0 || skip_layernorm > 3) return COEVO_ERR_ARG;
    if (n_children == 0) return COEVO_OK;
    const dim3 grid(quad_blocks(fc_stride(D)), (unsigned)n_children);
    hipLaunchKernelGGL(fc_perturb_kernel, grid, dim3(256), 0, (hipStream_t)stream, parent_slab, parent_idx,
                       child_slab, child_first, D, sigma_dev, seed, stream_lo_first, stream_hi, skip_layernorm, gen_dev,
                       dist_ref, dist_partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc_perturb(const float *parent_slab, const int32_t *parent_idx, float *child_slab,
                                int child_first, int n_children, int D, const float *sigma_dev, uint64_t seed,
                                uint32_t stream_lo_first, uint32_t stream_hi, int skip_layernorm, void *stream)
{
    return coevo_fc_perturb_dist(parent_slab, parent_idx, child_slab, child_first, n_children, D, sigma_dev, seed,
                                 stream_lo_first, stream_hi, skip_layernorm, nullptr, nullptr, nullptr, stream);
}

extern "C" int coevo_fc_perturb_gen(const float *parent_slab, const int32_t *parent_idx, float *child_slab,
                                    int child_first, int n_children, int D, const float *sigma_dev, uint64_t seed,
                                    uint32_t stream_lo_first, uint32_t stream_hi, int skip_layernorm,
                                    const int32_t *gen_dev, void *stream)
{
    return coevo_fc_perturb_dist(parent_slab, parent_idx, child_slab, child_first, n_children, D, sigma_dev, seed,
                                 stream_lo_first, stream_hi, skip_layernorm, gen_dev, nullptr, nullptr, stream);
}

extern "C" int coevo_fc_perturb_flags(const float *parent_slab, const int32_t *parent_idx, float *child_slab,
                                      int child_first, int n_children, int D, const float *sigma_dev, uint64_t seed,
                                      uint32_t stream_lo_first, uint32_t stream_hi, int flags, void *stream)
{
    if (flags < 0 || flags > 3) return COEVO_ERR_ARG;
    return coevo_fc_perturb_dist(parent_slab, parent_idx, child_slab, child_first, n_children, D, sigma_dev, seed,
                                 stream_lo_first, stream_hi, flags, nullptr, nullptr, nullptr, stream);
}

extern "C" int coevo_fc_perturb_dist_multi(const coevo_fc_perturb_job *jobs, int n_jobs, uint64_t seed, int skip_layernorm,
                                           const int32_t *gen_dev, void *stream)
{
    if (!jobs || n_jobs < 1 || n_jobs > COEVO_MAX_JOBS || skip_layernorm < 0 || skip_layernorm > 3) return COEVO_ERR_ARG;
    PerturbJobs pj{};
    unsigned gx = 0, gy = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const coevo_fc_perturb_job &j = jobs[i];
        if (!perturb_job_ok(j)) return COEVO_ERR_ARG;
        pj.j[i] = j;
        const unsigned nb = quad_blocks(fc_stride(j.D));
        gx = nb > gx ? nb : gx;
        gy = (unsigned)j.n_children > gy ? (unsigned)j.n_children : gy;
    }
    if (gy == 0) return COEVO_OK;
    hipLaunchKernelGGL(fc_perturb_multi_kernel, dim3(gx, gy, (unsigned)n_jobs), dim3(256), 0, (hipStream_t)stream, pj, seed,
                       skip_layernorm, gen_dev);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc_rebuild_elites(const float *elite_prev, const int32_t *order, float *elite_new, int E, int D,
                                       const float *sigma_prev_dev, uint64_t seed, uint32_t stream_hi_prev,
                                       const int32_t *gen_dev, void *stream)
{
    if (!elite_prev || !order || !elite_new || !sigma_prev_dev || !fc_dim_ok(D) || E <= 0 || E > 65535)
        return COEVO_ERR_ARG;
    if (elite_prev == elite_new) return COEVO_ERR_ARG;  // elite e reads several previous elites: never in place
    const dim3 grid(quad_blocks(fc_stride(D)), (unsigned)E);
    hipLaunchKernelGGL(fc_rebuild_elites_kernel, grid, dim3(256), 0, (hipStream_t)stream, elite_prev, order, elite_new,
                       E, D, sigma_prev_dev, seed, stream_hi_prev, gen_dev);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

/* dst[dst_first + i] = src[src_idx[i]] for nets of any layout (stride floats apart, a multiple of 4) */
extern "C" int coevo_net_gather(const float *src_slab, const int32_t *src_idx, float *dst_slab, int dst_first, int n,
                                int64_t stride_floats, void *stream)
{
    if (!src_slab || !src_idx || !dst_slab || n < 0 || dst_first < 0 || n > 65535 || stride_floats <= 0 ||
        (stride_floats & 3))
        return COEVO_ERR_ARG;
    if (n == 0) return COEVO_OK;
    const dim3 grid(quad_blocks(stride_floats), (unsigned)n);
    hipLaunchKernelGGL(fc_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, src_slab, src_idx, dst_slab,
                       dst_first, stride_floats);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc_gather(const float *src_slab, const int32_t *src_idx, float *dst_slab, int dst_first,
                               int n, int D, void *stream)
{
    if (!src_slab || !src_idx || !dst_slab || !fc_dim_ok(D) || n < 0 || dst_first < 0 || n > 65535)
        return COEVO_ERR_ARG;
    return coevo_net_gather(src_slab, src_idx, dst_slab, dst_first, n, fc_stride(D), stream);
}

static int ga_promote_launch(const coevo_ga_promote_role *roles, int n_roles, int E, int hof, const float *sigma,
                             uint64_t seed, uint32_t stream_hi_prev, const int32_t *gen_dev, int32_t *tick, void *stream)
{
    GaPromoteArgs a{};
    if (!promote_roles(a, roles, n_roles, E, hof, false)) return COEVO_ERR_ARG;
    a.sigma = sigma; a.seed = seed; a.stream_hi_prev = stream_hi_prev; a.gen_dev = gen_dev; a.tick = tick;
    unsigned max_blocks = 0;
    for (int r = 0; r < n_roles; ++r) max_blocks = std::max(max_blocks, quad_blocks(fc_stride(roles[r].D)));
    hipLaunchKernelGGL(ga_promote_kernel, dim3(max_blocks, (unsigned)n_roles), dim3(256), 0, (hipStream_t)stream, a);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_ga_promote(const coevo_ga_promote_role *roles, int n_roles, int E, int hof, void *stream)
{
    return ga_promote_launch(roles, n_roles, E, hof, nullptr, 0, 0, nullptr, nullptr, stream);
}

// ... with coevo_counter_add(counter, 1) in the same launch (the last launch of a device-resident generation's tail)
extern "C" int coevo_ga_promote_tick(const coevo_ga_promote_role *roles, int n_roles, int E, int hof, int32_t *counter,
                                     void *stream)
{
    if (!counter) return COEVO_ERR_ARG;
    return ga_promote_launch(roles, n_roles, E, hof, nullptr, 0, 0, nullptr, counter, stream);
}

// ... and the Hall of Fame's tile-major W2 twins kept in the same launch (the pipelined one-GPU loop, COEVO_TASK_TILED)
extern "C" int coevo_ga_promote_tick_tiled(const coevo_ga_promote_role *roles, int n_roles, int E, int hof, int32_t *counter,
                                           float *w2_twins, void *stream)
{
    if (!counter || !w2_twins || !aligned16(w2_twins)) return COEVO_ERR_ARG;
    GaPromoteArgs a{};
    if (!promote_roles(a, roles, n_roles, E, hof, true)) return COEVO_ERR_ARG;
    a.tick = counter;
    unsigned max_blocks = 0;
    for (int r = 0; r < n_roles; ++r) max_blocks = std::max(max_blocks, quad_blocks(fc_stride(roles[r].D)));
    hipLaunchKernelGGL(ga_promote_tiled_kernel, dim3(max_blocks, (unsigned)n_roles), dim3(256), 0, (hipStream_t)stream, a, w2_twins);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_fc_w2_tile_major(const float *src, float *dst, int n_nets, int D, void *stream)
{
    if (!src || !dst || !aligned16(src) || !aligned16(dst) || !fc_dim_ok(D) || n_nets < 0 || n_nets > 65535) return COEVO_ERR_ARG;
    if (n_nets == 0) return COEVO_OK;
    hipLaunchKernelGGL(fc_w2_tile_major_kernel, dim3((unsigned)(W2_FLOATS / 1024), (unsigned)n_nets), dim3(256), 0,
                       (hipStream_t)stream, src, dst, fc_stride(D), fc_off_w2(D));
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

// Promotion with the elites REBUILT in the same launch (a population-sharded run: a rank holds only its own individuals, so
// the new elites - individuals order[k] of the generation just evaluated - are regenerated from last generation's elites and
// the counter-based noise their children were bred with: genetic_algorithm.py:232-252 without a weight crossing xGMI).
// Replaces, per role, coevo_fc_gather (elite -> elite_prev) + coevo_fc_rebuild_elites + the coevo_ga_promote that followed:
// roles with elites_from_pop == 0 rebuild in place from `elite`, roles with elites_from_pop != 0 are promoted as usual.
// sigma: device [n_roles] floats (what the previous generation's children were bred with); noise stream of role r:
// stream_hi_prev + r (+ 4 (g - 1) when gen_dev is given).
extern "C" int coevo_ga_promote_rebuild(const coevo_ga_promote_role *roles, int n_roles, int E, int hof, const float *sigma,
                                        uint64_t seed, uint32_t stream_hi_prev, const int32_t *gen_dev, void *stream)
{
    if (!sigma) return COEVO_ERR_ARG;
    for (int r = 0; roles && r < n_roles && r < 3; ++r)
        if (!roles[r].elites_from_pop && !roles[r].order) return COEVO_ERR_ARG;
    return ga_promote_launch(roles, n_roles, E, hof, sigma, seed, stream_hi_prev, gen_dev, nullptr, stream);
}

extern "C" int coevo_es_update(float *theta_slab_net, const float *pert_slab, int D, const float *fitness, int n,
                               const float *sigma_dev, float lr, void *stream)
{
    if (!theta_slab_net || !pert_slab || !fitness || !sigma_dev || !fc_dim_ok(D) || n <= 0) return COEVO_ERR_ARG;
    const dim3 grid(quad_blocks(fc_stride(D)));
    hipLaunchKernelGGL(es_update_kernel, grid, dim3(256), 0, (hipStream_t)stream, theta_slab_net, pert_slab, D,
                       fitness, n, sigma_dev, lr);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

static int es_partial_launch(const float *theta_net, const float *pert_slab_local, int ind_first, int64_t stride,
                             const float *fitness_all, int n_total, int chunks_total, int chunk_first, int n_chunks,
                             float *partial, void *stream)
{
    if (!theta_net || !pert_slab_local || !fitness_all || !partial) return COEVO_ERR_ARG;
    if (n_total <= 0 || chunks_total <= 0 || chunk_first < 0 || n_chunks <= 0 || chunk_first + n_chunks > chunks_total ||
        n_chunks > 65535 || ind_first < 0)
        return COEVO_ERR_ARG;
    // the caller's nets must start exactly where its first chunk starts
    if ((int64_t)chunk_first * n_total / chunks_total != ind_first) return COEVO_ERR_ARG;
    const dim3 grid(quad_blocks(stride), (unsigned)n_chunks);
    hipLaunchKernelGGL(es_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, theta_net, pert_slab_local, ind_first,
                       stride, fitness_all, n_total, chunks_total, chunk_first, partial);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

static int es_apply_launch(float *theta_net, const float *partials, int chunks_total, int chunks_per_block,
                           int64_t block_stride_floats, int64_t stride, SlabSkip skip, int n_total,
                           const float *sigma_dev, float lr, void *stream)
{
    if (!theta_net || !partials || !sigma_dev || n_total <= 0 || chunks_total <= 0 || chunks_per_block <= 0 ||
        block_stride_floats < 0 || (block_stride_floats & 3))
        return COEVO_ERR_ARG;
    const dim3 grid(quad_blocks(stride));
    hipLaunchKernelGGL(es_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, theta_net, partials, chunks_total,
                       chunks_per_block, block_stride_floats, stride, skip, n_total, sigma_dev, lr);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_es_partial(const float *theta_net, const float *pert_slab_local, int ind_first, int D,
                                const float *fitness_all, int n_total, int chunks_total, int chunk_first, int n_chunks,
                                float *partial, void *stream)
{
    if (!fc_dim_ok(D)) return COEVO_ERR_ARG;
    return es_partial_launch(theta_net, pert_slab_local, ind_first, fc_stride(D), fitness_all, n_total, chunks_total,
                             chunk_first, n_chunks, partial, stream);
}

extern "C" int coevo_es_apply(float *theta_net, const float *partials, int chunks_total, int chunks_per_block,
                              int64_t block_stride_floats, int D, int n_total, const float *sigma_dev, float lr,
                              void *stream)
{
    if (!fc_dim_ok(D)) return COEVO_ERR_ARG;
    const int64_t g1 = fc_off_g1(D), g2 = fc_off_g2(D);  // LayerNorm affine: never perturbed, never updated
    const SlabSkip skip{fc_params(D), g1, g1 + 2 * H1, g2, g2 + 2 * H2, 0, 0};
    return es_apply_launch(theta_net, partials, chunks_total, chunks_per_block, block_stride_floats, fc_stride(D), skip,
                           n_total, sigma_dev, lr, stream);
}

extern "C" int coevo_dqn_es_partial(const float *theta_net, const float *pert_slab_local, int ind_first, int C,
                                    int n_actions, const float *fitness_all, int n_total, int chunks_total,
                                    int chunk_first, int n_chunks, float *partial, void *stream)
{
    if (!dqn_shape_ok(C, n_actions)) return COEVO_ERR_ARG;
    return es_partial_launch(theta_net, pert_slab_local, ind_first, dqn_layout(C, n_actions).stride, fitness_all,
                             n_total, chunks_total, chunk_first, n_chunks, partial, stream);
}

extern "C" int coevo_dqn_es_apply(float *theta_net, const float *partials, int chunks_total, int chunks_per_block,
                                  int64_t block_stride_floats, int C, int n_actions, int n_total,
                                  const float *sigma_dev, float lr, void *stream)
{
    if (!dqn_shape_ok(C, n_actions)) return COEVO_ERR_ARG;
    const DqnLayout L = dqn_layout(C, n_actions);  // BatchNorm affine is not perturbable (Atari/deepqn.py:158-171)
    const SlabSkip skip{L.total, L.b1 + 32, L.w2, L.b2 + 64, L.w3, L.b3 + 64, L.wf};
    return es_apply_launch(theta_net, partials, chunks_total, chunks_per_block, block_stride_floats, L.stride, skip,
                           n_total, sigma_dev, lr, stream);
}

// ---- the noise contract, exposed: the round count and the generator itself (raw words and the Gaussians built from them),
// so that a binding / a resumed run can check what it is loading and the tests can hold the generator against published
// known-answer vectors (Random123's kat_vectors) and moment / correlation bounds, independently of the oracle.
namespace coevo {
__global__ void philox_raw_kernel(int rounds, const uint32_t *ctr_key, int n, uint32_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *c = ctr_key + 6 * (size_t)i;
    u32x4 o;
    if (rounds == 7) o = philox4x32<7>(c[0], c[1], c[2], c[3], c[4], c[5]);
    else o = philox4x32<10>(c[0], c[1], c[2], c[3], c[4], c[5]);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * (size_t)i + k] = o.v[k];
}

__global__ void philox_normal_kernel(uint64_t seed, uint32_t stream_lo, uint32_t stream_hi, uint32_t q_first, int n_quads,
                                     float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_quads) return;
    float z[4];
    philox_normal4(seed, stream_lo, stream_hi, q_first + (uint32_t)i, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * (size_t)i + k] = z[k];
}
}  // namespace coevo

extern "C" int coevo_noise_rounds(void) { return coevo::COEVO_NOISE_ROUNDS; }

extern "C" int coevo_philox4x32(int rounds, const uint32_t *ctr_key, int n, uint32_t *out, void *stream)
{
    if (!ctr_key || !out || n <= 0 || (rounds != 7 && rounds != 10)) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(coevo::philox_raw_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, rounds, ctr_key, n,
                       out);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_philox_normals(uint64_t seed, uint32_t stream_lo, uint32_t stream_hi, uint32_t q_first, int n_quads,
                                    float *out, void *stream)
{
    if (!out || n_quads <= 0) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(coevo::philox_normal_kernel, dim3((n_quads + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed,
                       stream_lo, stream_hi, q_first, n_quads, out);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

COEVO_DEFINE_TU_FLAGS(offspring)
