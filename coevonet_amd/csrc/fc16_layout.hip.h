// The fp16 slab of one FCNetwork (args.precision == "float16") and the rounding helpers of the float16 contract, shared by
// the facade forward (fc16.hip), the rollout's env-cycle kernel (fc16_rollout.hip) and the four float16 update units
// (fc16_offspring.hip, fc16_es.hip, dqn16_offspring.hip, dqn16_es.hip).  The layout is ABI.
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

// The float16 contract rounds to fp32 FIRST wherever it names an fp32 value: f16(f32(a) + b), f16(sigma * eps).  Left alone,
// hipcc may fold the multiply or add into the conversion that follows it (v_fma_mixlo_f16: the exact result rounded once to
// fp16), which skips that fp32 rounding - about one entry in 10^5 of sigma * eps differs.  The empty statement makes the fp32
// value a value of its own.  The rounding helpers below are the ones the four update units share.
__device__ __forceinline__ float f32_pin(float v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// f16r of a value an fmaf has just produced, the fp32 result pinned in a register first: left to itself the compiler fuses the
// pair into v_fma_mixlo_f16, a mixed-precision FMA that rounds the exact sum ONCE to fp16 - the contract (and the reference's
// half modules, which compute in fp32 and store half) rounds to fp32, then to fp16.  (The conv stack of dqn_conv.hip.h and the
// output row of dqn_common.hip.h round with it.)
__device__ __forceinline__ float f16r_after_fma(float v)
{
    asm("" : "+v"(v));
    return f16r(v);
}

// child entry = f16(f32(parent) + noise): the sum in fp32, rounded once to half
__device__ __forceinline__ float f16_child(float parent, float noise) { return f16r(f32_pin(parent + noise)); }
// noise16 = f16(noise32), noise32 = sigma * eps the fp32 number the perturb launch added
__device__ __forceinline__ float f16_noise16(float noise32) { return f16r(f32_pin(noise32)); }
// distance term d = f16(f32(a) - f32(b)), a and b fp16 values.  No pin: for a sum of two p-bit numbers, rounding through a format
// of at least 2p + 1 bits first is innocuous (fp32 has 24 >= 23), so d is the correctly rounded fp16 difference whatever form
// the compiler picks (v_pk_add_f16 today)
__device__ __forceinline__ float f16_diff(float a, float b) { return f16r(a - b); }
// theta' = f16(theta + upd16), upd16 = f16(scale16 * dot16), dot16 = f16(sum): every fp32 intermediate a value of its own
__device__ __forceinline__ float f16_new_theta(float theta, float sum, float scale16)
{
    const float dot16 = f32_pin(f16r(f32_pin(sum)));
    const float upd16 = f32_pin(f16r(f32_pin(scale16 * dot16)));
    return f16r(f32_pin(f32_pin(theta) + upd16));
}

// fp64 -> fp16 in ONE rounding (to nearest even): to fp32 with round-to-odd first, which the fp32 -> fp16 conversion then
// rounds as if it saw the fp64 value (fp32 carries more than two bits beyond fp16's eleven)
__device__ inline float f16_of_f64(double s)
{
    float f = (float)s;
    if ((double)f != s && !__builtin_isinf(f) && !__builtin_isnan(f)) {
        uint32_t b = __float_as_uint(f);
        if (__builtin_fabs((double)f) > __builtin_fabs(s)) b -= 1u;   // back to the truncated value
        f = __uint_as_float(b | 1u);                                    // sticky bit
    }
    return f16r(f);
}
__device__ inline bool bad_post_relu16(float y) { return __builtin_isnan(y) || (__builtin_isinf(y) && y > 0.0f); }

constexpr int F16_R = 8;   // rows per pass; a task of more rows (<= COEVO_FC_MAX_ROWS) makes several passes

}  // namespace coevo
