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

}  // namespace coevo
