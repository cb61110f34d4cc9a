// The 16-byte pieces of an fp16 slab net (fc16_layout.hip.h) and the counter-based noise of a piece, shared by the float16
// breeding launch (fc16_offspring.hip) and the float16 Co-ES update (fc16_es.hip): the update regenerates the children's
// noise through the very function the children were written with.
// A thread owns ONE 16-byte piece of the net: in W2h that is k = 8kb .. 8kb+7 of output column j = eight consecutive canonical
// indices = two Philox quads; W3h likewise; a W1h piece is eight outputs of one input k, eight canonical indices D apart (one
// Philox block each, 3.6 % of a net); a piece of the fp32 tail is one quad.
#pragma once
#include "coevo_common.hip.h"
#include "fc16_layout.hip.h"
#include "philox.hip.h"

namespace coevo {

constexpr int F16_W2_PIECES = (int)(F16_W1 / 4);   // 16384 pieces of W2h
__host__ __device__ constexpr int f16_half_pieces(int D) { return (int)(f16_off_b1(D) / 4); }   // W2h + W1h + W3h
__host__ __device__ constexpr int f16_pieces(int D) { return (int)(f16_stride(D) / 4); }
__host__ __device__ constexpr int f16_perturb_blocks(int D) { return (f16_pieces(D) + 255) / 256; }

// word w (>= f16_off_b1) of the fp32 tail: 0 = a bias (an fp16 value), 1 = LayerNorm affine, 2 = the stride's padding
__device__ __forceinline__ int f16_tail_kind(int w, int D)
{
    const int b1 = (int)f16_off_b1(D), b2 = (int)f16_off_b2(D), b3 = (int)f16_off_b3(D);
    if (w < b2) return (w - b1) < H1 ? 0 : 1;
    if (w < b3) return (w - b2) < H2 ? 0 : 1;
    return w < b3 + NACT ? 0 : 2;
}

// ... and its canonical flat index (w < f16_used(D)); the three tail sections start at multiples of four in both orders
__device__ __forceinline__ int f16_tail_flat(int w, int D)
{
    const int b1 = (int)f16_off_b1(D), b2 = (int)f16_off_b2(D), b3 = (int)f16_off_b3(D);
    if (w < b2) return (int)fc_off_b1(D) + (w - b1);
    if (w < b3) return (int)fc_off_b2(D) + (w - b2);
    return (int)fc_off_b3(D) + (w - b3);
}

// eps(seed, stream, p) alone: the Box-Muller pair that holds element p % 4 of Philox block p / 4 (the bits of
// philox_normal4's z[p % 4]; the other pair of the block is not evaluated)
__device__ __forceinline__ float philox_normal1(uint64_t seed, uint32_t slo, uint32_t shi, int p)
{
    const u32x4 o = philox4x32<COEVO_NOISE_ROUNDS>((uint32_t)(p >> 2), slo, shi, 0x636f6576u, (uint32_t)seed,
                                                   (uint32_t)(seed >> 32));
    const bool hi = (p & 2) != 0;
    float z0, z1;
    box_muller(hi ? o.v[2] : o.v[0], hi ? o.v[3] : o.v[1], z0, z1);
    return (p & 1) ? z1 : z0;
}

// noise32 of the eight entries of half piece u (< f16_half_pieces(D)) in noise stream (slo, shi), in slab order: sigma *
// eps(seed, stream, p) rounded to fp32, p the canonical index of the entry
__device__ __forceinline__ void f16_half_piece_noise(int u, int D, float sigma, uint64_t seed, uint32_t slo, uint32_t shi,
                                                     float noise[8])
{
    float z[8];
    const int w1_pieces = D * (H1 / 8);
    if (u < F16_W2_PIECES || u >= F16_W2_PIECES + w1_pieces) {
        // W2h piece (kb, j) = fc2.w[j][8kb .. 8kb+7]; W3h piece t = output.w flat 8t .. 8t+7: eight consecutive
        // canonical indices from a multiple of eight - two Philox blocks
        const int p0 = (u < F16_W2_PIECES)
                           ? (int)fc_off_w2(D) + (u & (H2 - 1)) * H1 + 8 * (u >> 8)
                           : (int)fc_off_w3(D) + 8 * (u - F16_W2_PIECES - w1_pieces);
        philox_normal4(seed, slo, shi, (uint32_t)(p0 >> 2), z);
        philox_normal4(seed, slo, shi, (uint32_t)(p0 >> 2) + 1u, z + 4);
    } else {
        // W1h[k][j0 .. j0+7] = fc1.w[j0 + i][k]: canonical (j0 + i) D + k, a Philox block each
        const int h0 = 8 * (u - F16_W2_PIECES), k = h0 >> 9, j0 = h0 & (H1 - 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = philox_normal1(seed, slo, shi, (j0 + i) * D + k);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) noise[i] = sigma * z[i];   // rounded first, then added (agent.py:28-29)
}

// ... and of the four words of piece u (>= f16_half_pieces(D)) of the fp32 tail, LayerNorm words included (the caller decides
// by f16_tail_kind which it uses); 0 in a piece that lies wholly in the stride's padding
__device__ __forceinline__ void f16_tail_piece_noise(int u, int D, float sigma, uint64_t seed, uint32_t slo, uint32_t shi,
                                                     float noise[4])
{
    const int w0 = 4 * u;
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (w0 < (int)f16_used(D)) philox_normal4(seed, slo, shi, (uint32_t)(f16_tail_flat(w0, D) >> 2), z);
#pragma unroll
    for (int i = 0; i < 4; ++i) noise[i] = sigma * z[i];
}

}  // namespace coevo
