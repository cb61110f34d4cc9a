// The counter-based noise of a 16-byte piece of the TILED fc1 block of an fp16 DeepQN slab (dqn16_layout.hip.h wft16), for the
// breeding launch of dqn16_tiled.hip.  Everything outside the fc1 block is dqn16_pieces.hip.h's.
// Entry j of piece (ob, S, T, lane (c = lane % 16, kk = lane / 16)) is fc1.w[64 ob + 16 T + c][32 S + 4 j + kk], canonical index
// p_j = dqn_flat_wf(C) + (64 ob + 16 T + c) * 3136 + 32 S + 4 j + kk.  dqn_flat_wf(C), 3136 and 32 S are multiples of four, so
// entry j is element kk of Philox quad p_0 / 4 + j: a piece touches EIGHT consecutive quads (the streamed piece: two) and keeps one
// normal of each.  The plain form: every thread draws its eight blocks and runs the Box-Muller half that holds element kk - the
// pair (o[0], o[1]) gives elements 0 / 1, (o[2], o[3]) elements 2 / 3 (philox_normal4).  The four lanes (c, 0 .. 3) that share
// a quad are 16 lanes apart in a piece run that does not start on a wave boundary (the fc1 block starts at piece L.wf / 4):
// sharing them would need the float32 kernel's thread-map shift, which moves the 256-piece blocks of the distance partials.
#pragma once
#include "dqn16_pieces.hip.h"

namespace coevo {

__device__ __forceinline__ void dq16_fc1_piece_noise_tiled(int u, const DqnLayout &L, int C, float sigma, uint64_t seed,
                                                           uint32_t slo, uint32_t shi, float noise[8])
{
    const int t = u - (int)(L.wf >> 2), lane = t & 63, T = (t >> 6) & 3, S = (t >> 8) % DQ16_SUPER, ob = (t >> 8) / DQ16_SUPER;
    const int c = lane & 15, kk = lane >> 4;
    const uint32_t q0 = (uint32_t)(((int)dqn_flat_wf(C) + (64 * ob + 16 * T + c) * DQ_FC1_IN + 32 * S) >> 2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const u32x4 o = philox_noise_block(seed, slo, shi, q0 + (uint32_t)j);
        float z0, z1;
        box_muller(kk < 2 ? o.v[0] : o.v[2], kk < 2 ? o.v[1] : o.v[3], z0, z1);
        noise[j] = sigma * ((kk & 1) ? z1 : z0);
    }
}

}  // namespace coevo
