// The steps that the float16 update kernels of the FC nets (fc16_offspring.hip, fc16_es.hip) and of the DeepQN nets
// (dqn16_offspring.hip, dqn16_es.hip) run identically on a thread's 16-byte piece, each written once.  What differs between
// the families is layout: which pieces hold eight halves, which words of a four-word piece count or move, where a piece's
// floats start in a chunk partial.  The callers answer those; the roundings are f16_child / f16_noise16 / f16_diff /
// f16_new_theta of fc16_layout.hip.h.
#pragma once
#include "coevo_common.hip.h"
#include "fc16_layout.hip.h"

namespace coevo {

// squared distance of two pieces of eight halves: d = f16(f32(a) - f32(b)), d * d accumulated in fp64 in slab order
__device__ __forceinline__ double f16_d2_halves(const uint4 &a, const uint4 &b)
{
    _Float16 ha[8], hb[8];
    __builtin_memcpy(ha, &a, sizeof(ha));
    __builtin_memcpy(hb, &b, sizeof(hb));
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float d = f16_diff((float)ha[i], (float)hb[i]);
        d2 += (double)d * (double)d;
    }
    return d2;
}

// ... and of two pieces of four fp32 words that hold fp16 values; word i counts where counts(i)
template <class Counts>
__device__ __forceinline__ double f16_d2_words(const uint4 &a, const uint4 &b, const Counts &counts)
{
    float fa[4], fb[4];
    __builtin_memcpy(fa, &a, sizeof(fa));
    __builtin_memcpy(fb, &b, sizeof(fb));
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (counts(i)) {
            const float d = f16_diff(fa[i], fb[i]);
            d2 += (double)d * (double)d;
        }
    }
    return d2;
}

// acc[i] = fmaf(f32(fit16), f32(noise16[i]), acc[i]): one individual's term of a chunk sum
template <int N>
__device__ __forceinline__ void f16_es_accumulate(float (&acc)[N], float f, const float (&noise32)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = __builtin_fmaf(f, f16_noise16(noise32[i]), acc[i]);
}

// the chunk partials of a piece (pp: its floats in chunk 0, the chunks pitch floats apart) added left to right in fp32
__device__ __forceinline__ void f16_chunk_total8(const float *pp, int64_t pitch, int chunks_total, float sum[8])
{
    float4 lo = reinterpret_cast<const float4 *>(pp)[0], hi = reinterpret_cast<const float4 *>(pp)[1];
    for (int c = 1; c < chunks_total; ++c) {
        const float4 a = reinterpret_cast<const float4 *>(pp + c * pitch)[0];
        const float4 b = reinterpret_cast<const float4 *>(pp + c * pitch)[1];
        lo.x = lo.x + a.x; lo.y = lo.y + a.y; lo.z = lo.z + a.z; lo.w = lo.w + a.w;
        hi.x = hi.x + b.x; hi.y = hi.y + b.y; hi.z = hi.z + b.z; hi.w = hi.w + b.w;
    }
    sum[0] = lo.x; sum[1] = lo.y; sum[2] = lo.z; sum[3] = lo.w;
    sum[4] = hi.x; sum[5] = hi.y; sum[6] = hi.z; sum[7] = hi.w;
}

__device__ __forceinline__ void f16_chunk_total4(const float *pp, int64_t pitch, int chunks_total, float sum[4])
{
    float4 t = reinterpret_cast<const float4 *>(pp)[0];
    for (int c = 1; c < chunks_total; ++c) {
        const float4 a = reinterpret_cast<const float4 *>(pp + c * pitch)[0];
        t.x = t.x + a.x; t.y = t.y + a.y; t.z = t.z + a.z; t.w = t.w + a.w;
    }
    sum[0] = t.x; sum[1] = t.y; sum[2] = t.z; sum[3] = t.w;
}

// theta' of a piece of eight halves / of four words, of which word i moves where moves[i]
__device__ __forceinline__ uint4 f16_apply_halves(const uint4 &tv, const float (&sum)[8], float scale16)
{
    _Float16 hin[8], hout[8];
    __builtin_memcpy(hin, &tv, sizeof(hin));
#pragma unroll
    for (int i = 0; i < 8; ++i) hout[i] = (_Float16)f16_new_theta((float)hin[i], sum[i], scale16);
    uint4 ov;
    __builtin_memcpy(&ov, hout, sizeof(hout));
    return ov;
}

__device__ __forceinline__ uint4 f16_apply_words(const uint4 &tv, const float (&sum)[4], float scale16, const bool (&moves)[4])
{
    float in[4], out[4];
    __builtin_memcpy(in, &tv, sizeof(in));
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = moves[i] ? f16_new_theta(in[i], sum[i], scale16) : in[i];
    uint4 ov;
    __builtin_memcpy(&ov, out, sizeof(out));
    return ov;
}

// ---- host: the argument checks that the two *_es16_partial and the two *_es16_apply entry points share ---------------
constexpr int ES16_MAX_CHUNKS = 64;

inline bool es16_partial_args_ok(const float *fitness, const float *sigma_dev, const float *partial, bool shape_ok, int n_total,
                                 int chunks_total)
{
    if (!fitness || !sigma_dev || !partial || !shape_ok || n_total < 1) return false;
    return chunks_total >= 1 && chunks_total <= ES16_MAX_CHUNKS && aligned16(partial);
}

inline bool es16_apply_args_ok(const void *theta16_net, const float *partial, const float *sigma_dev, bool shape_ok, int n_total,
                               int chunks_total)
{
    if (!theta16_net || !partial || !sigma_dev || !shape_ok || n_total < 1) return false;
    return chunks_total >= 1 && chunks_total <= ES16_MAX_CHUNKS && aligned16(theta16_net) && aligned16(partial);
}

}  // namespace coevo
