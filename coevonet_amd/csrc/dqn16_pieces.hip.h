// The 16-byte pieces of an fp16 DeepQN slab net (dqn16_layout.hip.h) and the counter-based noise of a piece, shared by the
// float16 DeepQN breeding launch (dqn16_offspring.hip) and the float16 DeepQN Co-ES update (dqn16_es.hip): the update
// regenerates the children's noise through the very functions the children were written with (fc16_pieces.hip.h does the same
// for the FC nets).
// A thread owns ONE 16-byte piece of the net.  In the fc1 block ([8][392][64][8] halves, 91 % of the words) that is eight
// consecutive canonical indices from a multiple of eight = two aligned Philox quads; everywhere else it is four fp32 words that
// hold fp16 values and map through dqn16_word_to_flat - the conv weights sit in conv16_mfma's lane order, so such a piece can
// need four Philox blocks.
#pragma once
#include "dqn16_layout.hip.h"
#include "f16_steps.hip.h"
#include "philox.hip.h"

namespace coevo {

__device__ __forceinline__ int dq16_pieces(const DqnLayout &L) { return (int)(L.stride >> 2); }
__device__ __forceinline__ bool dq16_fc1_piece(int u, const DqnLayout &L) { return 4 * (int64_t)u >= L.wf && 4 * (int64_t)u < L.bf; }
// workgroups of 256 pieces that cover a net
inline unsigned dqn16_blocks(int C, int n) { return quad_blocks(dqn16_layout(C, n).stride); }

// word s outside the fc1 block takes noise: a parameter (dqn16_word_to_flat >= 0) and, under skip_bn, not BatchNorm affine
__device__ __forceinline__ bool dq16_word_moves(int64_t s, const DqnLayout &L, bool skip_bn)
{
    return s < L.total && !(skip_bn && dqn_slab_is_batchnorm(s, L));
}

// noise32 of the eight entries of fc1 piece u in noise stream (slo, shi), in slab order: sigma * eps(seed, stream, p) rounded
// to fp32, p the canonical index of the entry.  Piece (ob, o, l) = fc1.w[64 ob + l][8 o .. 8 o + 7]: never BatchNorm, never padding
__device__ __forceinline__ void dq16_fc1_piece_noise(int u, const DqnLayout &L, int C, float sigma, uint64_t seed, uint32_t slo,
                                                     uint32_t shi, float noise[8])
{
    const int t = u - (int)(L.wf >> 2), l = t & 63, o = (t >> 6) % DQ16_OCTETS, ob = (t >> 6) / DQ16_OCTETS;
    const uint32_t q0 = (uint32_t)(((int)dqn_flat_wf(C) + (ob * 64 + l) * DQ_FC1_IN + 8 * o) >> 2);
    float z[8];
    philox_normal4(seed, slo, shi, q0, z);
    philox_normal4(seed, slo, shi, q0 + 1u, z + 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) noise[i] = sigma * z[i];
}

// canonical indices of the four words of piece u outside the fc1 block (-1: the stride's padding).  They depend on no stream:
// mapped once per thread
__device__ __forceinline__ void dq16_word_piece_flat(int u, int C, int n_actions, int64_t p[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = dqn16_word_to_flat(4 * (int64_t)u + i, C, n_actions);
}

// ... and their noise32 in one stream, 0 where want[i] is false.  A word that is not wanted costs no Philox block; of the
// blocks a piece needs the last one drawn is kept, as in the generic branch of dqn_perturb_kernel
__device__ __forceinline__ void dq16_word_piece_noise(const int64_t (&p)[4], const bool (&want)[4], float sigma, uint64_t seed,
                                                      uint32_t slo, uint32_t shi, float noise[4])
{
    float zz[4];
    int64_t have = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        noise[i] = 0.0f;
        if (!want[i]) continue;
        const int64_t q = p[i] >> 2;
        if (q != have) { philox_normal4(seed, slo, shi, (uint32_t)q, zz); have = q; }
        const int e = (int)(p[i] & 3);
        const float zi = e == 0 ? zz[0] : (e == 1 ? zz[1] : (e == 2 ? zz[2] : zz[3]));   // (no runtime-indexed array)
        noise[i] = sigma * zi;
    }
}

// squared distance of piece u of net a to the same piece of net b: the piece's entries in slab order, padding left out.  The
// fc1 block's two forms hold the same halves in pieces of eight, so two nets of ONE form give the same terms, grouped otherwise
__device__ __forceinline__ double dq16_piece_d2(const uint4 &a, const uint4 &b, int u, const DqnLayout &L)
{
    if (dq16_fc1_piece(u, L)) return f16_d2_halves(a, b);
    return f16_d2_words(a, b, [&](int i) { return 4 * (int64_t)u + i < L.total; });   // dqn16_word_to_flat >= 0
}

// the arguments of one breeding launch (coevo_dqn16_perturb_dist and its tiled twin take the same ones)
struct Dq16PerturbArgs {
    const uint32_t *parent_slab;
    const int32_t *parent_idx;
    uint32_t *child_slab;
    int child_first, C, n_actions;
    const float *sigma_dev;
    uint64_t seed;
    uint32_t stream_lo_first, stream_hi;
    int flags;
    const int32_t *gen_dev;
    int gen_bias;
    const uint32_t *dist_ref;
    double *dist_partial;
};

// The body of the breeding launch, grid (dqn16_blocks, n_children): workgroup (bx, c) writes pieces 256 bx .. 256 bx + 255 of
// child c and the block's distance partial.  fc1_noise(u, L, C, sigma, seed, slo, shi, noise[8]) is the noise of an fc1 piece
// in slab order: the one thing the slab's fc1 form changes.
template <class Fc1Noise>
__device__ __forceinline__ void dq16_perturb_dist_body(const Dq16PerturbArgs &a, double *scratch, const Fc1Noise &fc1_noise)
{
    uint32_t stream_hi = a.stream_hi;
    if (a.gen_dev) stream_hi += 4u * (uint32_t)(*a.gen_dev + a.gen_bias);   // generation-indexed noise stream without a host argument
    const int c = blockIdx.y, bx = blockIdx.x, C = a.C, n_actions = a.n_actions, flags = a.flags;
    const uint32_t slo = a.stream_lo_first + (uint32_t)c;
    const DqnLayout L = dqn16_layout(C, n_actions);
    const int u = bx * 256 + (int)threadIdx.x;
    double d2 = 0.0;
    if (u < dq16_pieces(L)) {
        const uint4 pv = reinterpret_cast<const uint4 *>(a.parent_slab + (int64_t)a.parent_idx[c] * L.stride)[u];
        uint4 ov = pv;
        if (!(flags & COEVO_DQP_COPY)) {
            const float sigma = *a.sigma_dev;
            if (dq16_fc1_piece(u, L)) {
                float noise[8];
                fc1_noise(u, L, C, sigma, a.seed, slo, stream_hi, noise);
                _Float16 hin[8], hout[8];
                __builtin_memcpy(hin, &pv, sizeof(hin));
#pragma unroll
                for (int i = 0; i < 8; ++i) hout[i] = (_Float16)f16_child((float)hin[i], noise[i]);
                __builtin_memcpy(&ov, hout, sizeof(hout));
            } else {
                int64_t p[4];
                bool want[4];
                dq16_word_piece_flat(u, C, n_actions, p);
#pragma unroll
                for (int i = 0; i < 4; ++i) want[i] = dq16_word_moves(4 * (int64_t)u + i, L, (flags & COEVO_DQP_SKIP_BN) != 0);
                float in[4], out[4], noise[4];
                dq16_word_piece_noise(p, want, sigma, a.seed, slo, stream_hi, noise);
                __builtin_memcpy(in, &pv, sizeof(in));
#pragma unroll
                for (int i = 0; i < 4; ++i) out[i] = want[i] ? f16_child(in[i], noise[i]) : in[i];
                __builtin_memcpy(&ov, out, sizeof(out));
            }
        }
        // a plain store: the rollout reads the child next
        if (a.child_slab) reinterpret_cast<uint4 *>(a.child_slab + (int64_t)(a.child_first + c) * L.stride)[u] = ov;
        if (a.dist_partial) d2 = dq16_piece_d2(ov, reinterpret_cast<const uint4 *>(a.dist_ref)[u], u, L);
    }
    if (a.dist_partial) {   // uniform over the launch
        const double tot = block_sum_f64(d2, scratch);
        if (threadIdx.x == 0) a.dist_partial[(size_t)c * gridDim.x + bx] = tot;
    }
}

// ---- host: the argument checks of the two breeding entry points.  COEVO_OK: launch; COEVO_ERR_ARG; 1: nothing to do
inline int dqn16_perturb_args(const void *parent_slab, const int32_t *parent_idx, const void *child_slab, int child_first,
                              int n_children, int C, int n_actions, const float *sigma_dev, int flags, const void *dist_ref,
                              const double *dist_partial)
{
    if ((dist_ref == nullptr) != (dist_partial == nullptr)) return COEVO_ERR_ARG;
    if (!dqn_shape_ok(C, n_actions)) return COEVO_ERR_ARG;   // (any bit or-ed into C fails here)
    if (flags & ~(COEVO_DQP_SKIP_BN | COEVO_DQP_COPY)) return COEVO_ERR_ARG;   // antithetic / from-order: not built for fp16
    const bool copy = (flags & COEVO_DQP_COPY) != 0;
    if (!parent_slab || !parent_idx || (!sigma_dev && !copy)) return COEVO_ERR_ARG;
    if (!child_slab && !(copy && dist_partial)) return COEVO_ERR_ARG;   // NULL child: the distance of existing nets only
    if (!aligned16(parent_slab) || !aligned16(child_slab) || !aligned16(dist_ref)) return COEVO_ERR_ARG;
    if (n_children < 0 || child_first < 0 || n_children > 65535) return COEVO_ERR_ARG;
    return n_children == 0 ? 1 : COEVO_OK;
}

}  // namespace coevo
