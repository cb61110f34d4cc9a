// The tile-pair and slab arithmetic of the all-pairs distance launches, shared by the fp32 kernel (sharing.hip) and the fp16
// kernel (fc16_sharing.hip): a workgroup takes 32 i-nets x 32 j-nets (tile row <= tile column) and a slab of the parameter axis,
// which is cut into PW_CHUNK-word pieces; partial sums go to scratch [slab][i][j] (i < j).
#pragma once
#include "coevo_common.hip.h"

namespace coevo {

constexpr int PW_TILE = 32;      // nets per tile side
constexpr int PW_CHUNK = 64;     // 32-bit words per net and LDS piece (both strides are multiples of 64)
constexpr int PW_ROW = PW_CHUNK + 4;
constexpr int PW_MAX_SLABS = 64;
constexpr int PW_TARGET_WGS = 2048;   // ~8 workgroups of 4 waves per CU

static inline int pw_tiles(int n) { return (n + PW_TILE - 1) / PW_TILE; }
static inline int pw_tile_pairs(int n) { return pw_tiles(n) * (pw_tiles(n) + 1) / 2; }
// slabs of the parameter axis (`chunks` pieces of PW_CHUNK words): enough workgroups at a small population (pop 200: 28 tile
// pairs), one slab at a large one
static inline int pw_slabs_of(int n, int chunks)
{
    int s = (PW_TARGET_WGS + pw_tile_pairs(n) - 1) / pw_tile_pairs(n);
    s = s > PW_MAX_SLABS ? PW_MAX_SLABS : s;
    return s > chunks ? chunks : s;
}

// what workgroup (blockIdx.x = tile pair, blockIdx.y = slab) covers: nets i0 .. i0 + 31 against j0 .. j0 + 31, pieces
// [c_lo, c_hi) of `chunks`
struct PwBlock {
    int i0, j0, c_lo, c_hi, slab;
};
__device__ __forceinline__ PwBlock pw_block(int n, int chunks, int n_slabs)
{
    const int nb = (n + PW_TILE - 1) / PW_TILE;
    int bi = 0, rem = (int)blockIdx.x;   // tile pair number -> (bi, bj), bi <= bj, row by row of the upper triangle
    while (rem >= nb - bi) { rem -= nb - bi; ++bi; }
    const int bj = bi + rem, slab = (int)blockIdx.y;
    return PwBlock{bi * PW_TILE, bj * PW_TILE, (int)((int64_t)slab * chunks / n_slabs),
                   (int)((int64_t)(slab + 1) * chunks / n_slabs), slab};
}

}  // namespace coevo
