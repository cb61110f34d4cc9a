// Device pieces of the baseline opponents (include/coevo_baseline.h) that more than one translation unit needs: the
// scripted-action statement, the geometry of a PPO policy net, its non-finite tests and the first-maximum scan.  baseline.hip
// plays them one seat / one row per thread; gauntlet.hip plays them inside its one-launch game loop.
#pragma once
#include "coevo_common.hip.h"
#include "philox.hip.h"

#include "../../include/coevo_baseline.h"

namespace coevo {

constexpr int MLP_H = COEVO_MLP_H, MLP_NACT = COEVO_MLP_NACT, MLP_TILE = COEVO_MLP_ROW_TILE;
__host__ __device__ constexpr int mlp_params(int D) { return MLP_H * D + MLP_H + MLP_H * MLP_H + MLP_H + MLP_NACT * MLP_H + MLP_NACT; }
__host__ __device__ constexpr int mlp_stride(int D) { return (mlp_params(D) + 3) / 4 * 4; }
constexpr int MLP_LDS_FLOATS = mlp_stride(10);

// scripted_action(kind, arg, seed, ordinal, slot, k, n_actions) of coevo_baseline.h -> false for a seat that plays nothing (an
// unknown kind, a periodic start below 0, a constant outside 0 .. n_actions - 1).  ordinal_of() is called by a random seat only.
template <class OrdinalOf>
__device__ __forceinline__ bool scripted_action(int kind, int arg, uint32_t seed_lo, uint32_t seed_hi, OrdinalOf ordinal_of,
                                                int slot, uint32_t k, int n_actions, int &action_out)
{
    int action;
    if (kind == COEVO_BL_RANDOM) {
        const uint64_t ordinal = ordinal_of();
        const u32x4 o = philox4x32_10((uint32_t)ordinal, (uint32_t)(ordinal >> 32), k, (uint32_t)slot, seed_lo, seed_hi);
        action = (int)(((uint64_t)o.v[0] * (uint64_t)n_actions) >> 32);
    } else if (kind == COEVO_BL_PERIODIC) {
        if (arg < 0) return false;
        action = (int)(((uint64_t)arg + (uint64_t)k) % (uint64_t)n_actions);
    } else if (kind == COEVO_BL_CONSTANT) {
        if (arg < 0 || arg >= n_actions) return false;
        action = arg;
    } else {
        return false;
    }
    action_out = action;
    return true;
}

__device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
// the largest |bits| of a layer's outputs, taken as each output appears (the empty asm pins the running maximum there:
// left to itself the compiler gathers the 64 tests at the end of the layer and keeps every pre-ReLU value alive for them)
__device__ __forceinline__ void track_magnitude(uint32_t &m, float v)
{
    const uint32_t b = __float_as_uint(v) & 0x7fffffffu;
    m = b > m ? b : m;
    asm volatile("" : "+v"(m));
}
__device__ __forceinline__ bool magnitude_not_finite(uint32_t m) { return m >= 0x7f800000u; }
__device__ __forceinline__ float relu_plus_zero(float v) { return v > 0.0f ? v : 0.0f; }   // NaN and -0 give +0

__device__ __forceinline__ int first_max(const float (&logit)[MLP_NACT])
{
    int best = 0;
    float cur = logit[0];
#pragma unroll
    for (int c = 1; c < MLP_NACT; ++c)
        if (logit[c] > cur) { cur = logit[c]; best = c; }
    return best;
}

}  // namespace coevo
