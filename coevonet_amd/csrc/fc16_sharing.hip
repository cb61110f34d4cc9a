// Population sharing over float16 nets (include/coevo_sharing16.h): all pairwise distances of a population in the fp16 slab of
// fc16_layout.hip.h, each row what coevo_fc16_distance + coevo_fc16_distance_finalize give for that reference net.  The niche
// counts, the fitness and the ranking are sharing.hip's fp32 launches on the fp16-valued matrix.
//
// The float16 distance contract (DESIGN.md "float16 nets"): per Linear entry d = f16(f32(a) - f32(b)), d * d added in fp64,
// dist = f16(sqrt(sum)) in one rounding, stored as an fp32 word.  The launch is sharing.hip's (pairwise_tiles.hip.h):
//   * a workgroup takes 32 i-nets x 32 j-nets and a slab of the parameter axis; thread (ti, tj) of 16 x 16 keeps the pairs
//     {ti, ti + 16} x {tj, tj + 16}, so each 16-byte piece it reads from LDS feeds two pairs;
//   * 64 words of the 64 nets at a time go through LDS, rows padded to 68 words.  A piece of the half region (W2h, W1h, W3h) is
//     staged as it is: eight halves per 16 bytes.  A piece of the fp32 tail is staged as halves too - a bias word holds an fp16
//     value, so the conversion is exact -, four to 16 bytes and four +0.0 halves behind them; LayerNorm gamma / beta, the
//     stride's padding and the nets past n are ZEROED on the way in, so what those words hold never reaches the arithmetic;
//   * two terms per packed fp16 subtraction (v_pk_add_f16 with a negated operand): the fp16 difference of two fp16 values is
//     correctly rounded, and so is f16(f32(a) - f32(b)) (fc16_layout.hip.h f16_diff: fp32 has 24 >= 2 * 11 + 1 bits), so the
//     two are the same word.  d * d is exact in fp32 (22 significant bits at most; 65504^2 and 2^-48 are inside its range) and
//     is added to an fp64 accumulator that started at +0.0; a zeroed entry adds +0.0, which leaves it as it was;
//   * partial sums go to scratch [slab][i][j] (i < j), and a second launch adds them in slab order, takes the root, rounds it
//     once to fp16 (f16_of_f64) and writes dist[i][j] and dist[j][i] from the same word: symmetric bits, no atomics, a fixed
//     order for given (n, D).
#include "coevo_common.hip.h"
#include "fc16_layout.hip.h"
#include "fc16_pieces.hip.h"
#include "pairwise_tiles.hip.h"

#include "../../include/coevo_sharing16.h"

namespace coevo {

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

static_assert(f16_off_b1(8) % PW_CHUNK == 0 && f16_off_b1(10) % PW_CHUNK == 0, "a piece lies wholly in the half region or the tail");

static inline int pw16_chunks(int D) { return (int)(f16_stride(D) / PW_CHUNK); }
static inline int pw16_slabs(int n, int D) { return pw_slabs_of(n, pw16_chunks(D)); }

// one thread's four 16-byte pieces of an LDS piece: piece f = threadIdx.x + 256 m covers row f / 16 (0-31 the i-tile, 32-63 the
// j-tile), words 4 (f % 16) .. of the chunk starting at word s_chunk; every piece comes back as eight halves
__device__ __forceinline__ void pw16_load(const uint32_t *pop_slab, int n, int stride, int D, int i0, int j0, int s_chunk,
                                          uint4 (&v)[4])
{
    const bool tail = s_chunk >= (int)f16_off_b1(D);   // workgroup-uniform
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int f = (int)threadIdx.x + 256 * m;
        const int row = f >> 4, q = f & 15;
        const int net = (row < PW_TILE ? i0 + row : j0 + row - PW_TILE);
        const int s = s_chunk + 4 * q;
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (net < n) x = *reinterpret_cast<const uint4 *>(pop_slab + (int64_t)net * stride + s);
        if (tail) {
            float w[4];
            __builtin_memcpy(w, &x, sizeof(w));
            _Float16 h[8];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                h[c] = (_Float16)(f16_tail_kind(s + c, D) == 0 ? w[c] : 0.0f);
                h[4 + c] = (_Float16)0.0f;
            }
            __builtin_memcpy(&x, h, sizeof(h));
        }
        v[m] = x;
    }
}

// the eight terms of two pieces of eight halves, slab order, into one fp64 accumulator
__device__ __forceinline__ void pw16_acc8(const uint4 &a, const uint4 &b, double &acc)
{
    half2_t ha[4], hb[4];
    __builtin_memcpy(ha, &a, sizeof(ha));
    __builtin_memcpy(hb, &b, sizeof(hb));
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const half2_t d = hb[p] - ha[p];
        // d * d + 0 in fp32 straight from the fp16 halves (v_fma_mix_f32): exact, so it is the square, +0.0 included
        const float x = __builtin_fmaf((float)d.x, (float)d.x, 0.0f), y = __builtin_fmaf((float)d.y, (float)d.y, 0.0f);
        acc = acc + (double)x;
        acc = acc + (double)y;
    }
}

// grid (tile pair, slab); scratch[(slab * n + i) * n + j] for the pairs i < j of the tile pair
__global__ __launch_bounds__(256) void fc16_pairwise_partial_kernel(const uint32_t *pop_slab, int n, int D, int n_slabs,
                                                                     double *scratch)
{
    __shared__ uint4 sh[2 * PW_TILE][PW_ROW / 4];
    const int stride = (int)f16_stride(D);
    const PwBlock B = pw_block(n, stride / PW_CHUNK, n_slabs);
    const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;
    double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0;   // (ti, tj), (ti, tj + 16), (ti + 16, tj), (ti + 16, tj + 16)
    uint4 next[4];
    if (B.c_lo < B.c_hi) pw16_load(pop_slab, n, stride, D, B.i0, B.j0, B.c_lo * PW_CHUNK, next);
    for (int c = B.c_lo; c < B.c_hi; ++c) {
        __syncthreads();   // the previous piece has been read by every wave
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int f = (int)threadIdx.x + 256 * m;
            sh[f >> 4][f & 15] = next[m];
        }
        __syncthreads();
        if (c + 1 < B.c_hi) pw16_load(pop_slab, n, stride, D, B.i0, B.j0, (c + 1) * PW_CHUNK, next);
#pragma unroll 2
        for (int k = 0; k < PW_CHUNK / 4; ++k) {
            const uint4 a0 = sh[ti][k], a1 = sh[ti + 16][k];
            const uint4 b0 = sh[PW_TILE + tj][k], b1 = sh[PW_TILE + tj + 16][k];
            pw16_acc8(a0, b0, acc00);
            pw16_acc8(a0, b1, acc01);
            pw16_acc8(a1, b0, acc10);
            pw16_acc8(a1, b1, acc11);
        }
    }
    const double acc[2][2] = {{acc00, acc01}, {acc10, acc11}};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i = B.i0 + ti + 16 * a, j = B.j0 + tj + 16 * b;
            if (i < n && j < n && i < j) scratch[((size_t)B.slab * n + i) * n + j] = acc[a][b];
        }
}

// dist[i][j] = dist[j][i] = f16_of_f64(sqrt(partials of the pair (min, max) added in slab order from +0.0)); the diagonal +0.0
__global__ __launch_bounds__(256) void fc16_pairwise_finish_kernel(const double *scratch, int n, int n_slabs, float *dist)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * n) return;
    const int i = (int)(idx / n), j = (int)(idx % n);
    if (i == j) {
        dist[idx] = 0.0f;
        return;
    }
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double tot = 0.0;
    for (int s = 0; s < n_slabs; ++s) tot = tot + scratch[((size_t)s * n + lo) * n + hi];
    dist[idx] = f16_of_f64(sqrt(tot));
}

static bool pw16_shape_ok(int n, int D) { return n >= 1 && n <= COEVO_SHARING_MAX_POP && fc_dim_ok(D); }

}  // namespace coevo

using namespace coevo;

extern "C" int64_t coevo_fc16_pairwise_scratch_doubles(int n, int D)
{
    if (!pw16_shape_ok(n, D)) return COEVO_ERR_ARG;
    return (int64_t)pw16_slabs(n, D) * n * n;
}

extern "C" int coevo_fc16_pairwise_distance(const void *pop_slab, int n, int D, double *scratch, float *dist, void *stream)
{
    if (!pop_slab || !scratch || !dist || !pw16_shape_ok(n, D) || !aligned16(pop_slab) ||
        (reinterpret_cast<uintptr_t>(scratch) & 7u))
        return COEVO_ERR_ARG;
    const int n_slabs = pw16_slabs(n, D);
    hipLaunchKernelGGL(fc16_pairwise_partial_kernel, dim3(pw_tile_pairs(n), n_slabs), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const uint32_t *>(pop_slab), n, D, n_slabs, scratch);
    COEVO_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(fc16_pairwise_finish_kernel, dim3((unsigned)(((int64_t)n * n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, scratch, n, n_slabs, dist);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
