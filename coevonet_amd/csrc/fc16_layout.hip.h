// The fp16 slab of one FCNetwork (args.precision == "float16") and the rounding helpers of the float16 contract, shared by
// the facade forward (fc16.hip) and the rollout's env-cycle kernel (fc16_rollout.hip).  The layout is ABI.
#pragma once
#include "coevo_common.hip.h"

namespace coevo {

// ---- fp16 slab layout of one net, in 32-bit words (the unit of coevo_fc_task.net_off); every section 16-byte aligned --
//   W2h [64][256][8] half   fc2.weight: piece (kb, j) = k 8kb .. 8kb+7 of output column j, one 16-byte load; the 256
//                           lanes of a workgroup (one column each) read 4 KiB contiguous per k-block
//   W1h [D][512] half       fc1.weight transposed (k-major: a wavefront reads 64 consecutive outputs of one k)
//   W3h [5][256] half       output.weight, row-major
//   b1 g1 be1 [512], b2 g2 be2 [256], b3 [5]   fp32 (biases upcast - exact -, LayerNorm affine is fp32 in the reference)
// The stride is padded to a multiple of 64 words (256 bytes), like the fp32 slab.
constexpr int64_t F16_W1 = (int64_t)H1 * H2 / 2;  // 65536 words of W2h
__host__ __device__ constexpr int64_t f16_off_w3(int D) { return F16_W1 + (int64_t)D * H1 / 2; }
__host__ __device__ constexpr int64_t f16_off_b1(int D) { return f16_off_w3(D) + NACT * H2 / 2; }
__host__ __device__ constexpr int64_t f16_off_b2(int D) { return f16_off_b1(D) + 3 * H1; }
__host__ __device__ constexpr int64_t f16_off_b3(int D) { return f16_off_b2(D) + 3 * H2; }
__host__ __device__ constexpr int64_t f16_used(int D) { return f16_off_b3(D) + NACT; }
__host__ __device__ constexpr int64_t f16_stride(int D) { return (f16_used(D) + 63) / 64 * 64; }

__device__ inline float f16r(float v) { return (float)(_Float16)v; }
__device__ inline bool bad_post_relu16(float y) { return __builtin_isnan(y) || (__builtin_isinf(y) && y > 0.0f); }

constexpr int F16_R = 8;   // rows per pass; a task of more rows (<= COEVO_FC_MAX_ROWS) makes several passes

}  // namespace coevo
