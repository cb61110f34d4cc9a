// Population sharing (include/coevo_sharing.h): all pairwise distances of a population in one pass, the per-individual niche
// counts over them, and the GA fitness with its two switches (every Hall-of-Fame game / a share per individual).  Extension
// modes, NOT the reference's algorithm: genetic_algorithm.py:133 measures every individual against one stale agent (quirk Q3)
// and :140 keeps the last Hall-of-Fame game only (Q2); the function it calls, diversity_penalty
// (utils/game_logic_functions.py:12-37), is the niche count written here.
//
// Pairwise kernel.  Same arithmetic per entry as fc_distance_kernel (select.hip): df = w_j - w_i in fp32, its square exact in
// fp64, an fp64 sum.  VALU work - per pair and entry one v_sub_f32, one v_cvt_f64_f32, one v_fma_f64 - so the point is to read
// each net about n / 32 times instead of n times:
//   * a workgroup takes 32 i-nets x 32 j-nets (tile row <= tile column; the diagonal tile is computed once) and a slab of the
//     parameter axis; thread (ti, tj) of 16 x 16 keeps the four pairs {ti, ti + 16} x {tj, tj + 16} in registers, so each
//     16-byte piece it reads from LDS feeds two pairs;
//   * 64 entries of the 64 nets at a time go through LDS (rows padded to 68 floats: the 16 rows that a ds_read_b128 lane
//     group reads start 4 banks apart), the next piece's global loads in flight under the arithmetic;
//   * LayerNorm entries, the stride's padding and the rows past n are ZEROED on their way into LDS: 0 - 0 squares to +0.0,
//     which leaves an accumulator that started at +0.0 and only ever took squares exactly as it was - the inner loop has no
//     predicate, and what those words hold (NaN, 1e30) never reaches the arithmetic;
//   * partial sums go to scratch [slab][i][j] (i < j), and a second launch adds them in slab order, takes the root and writes
//     dist[i][j] and dist[j][i] from the same words: symmetric bits, no atomics, a fixed order for given (n, D).
#include "coevo_common.hip.h"
#include "pairwise_tiles.hip.h"

#include "../../include/coevo_sharing.h"

namespace coevo {

static inline int pw_slabs(int n, int D) { return pw_slabs_of(n, (int)(fc_stride(D) / PW_CHUNK)); }

// one thread's four 16-byte pieces of an LDS piece: piece f = threadIdx.x + 256 m covers row f / 16 (0-31 the i-tile, 32-63 the
// j-tile), entries 4 (f % 16) ..; excluded words (LayerNorm, padding, nets past n) come back as +0.0
// (slab positions fit 32 bits: the stride is ~140 000)
__device__ __forceinline__ void pw_load(const float *pop_slab, int n, int stride, int P, int g1, int g2, int i0, int j0,
                                        int s_chunk, float4 (&v)[4])
{
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int f = (int)threadIdx.x + 256 * m;
        const int row = f >> 4, q = f & 15;
        const int net = (row < PW_TILE ? i0 + row : j0 + row - PW_TILE);
        const int s = s_chunk + 4 * q;
        float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (net < n) x = *reinterpret_cast<const float4 *>(pop_slab + (int64_t)net * stride + s);
        float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int p = s + c;
            const bool ln = (p >= g1 && p < g1 + 2 * H1) || (p >= g2 && p < g2 + 2 * H2);
            if (p >= P || ln) e[c] = 0.0f;
        }
        v[m] = make_float4(e[0], e[1], e[2], e[3]);
    }
}

__device__ __forceinline__ void pw_fma4(const float4 &a, const float4 &b, double &acc)
{
    const float d0 = b.x - a.x, d1 = b.y - a.y, d2 = b.z - a.z, d3 = b.w - a.w;
    // (the square of an fp32 value is exact in fp64, so the fused form rounds exactly where `acc + d * d` does)
    acc = __builtin_fma((double)d0, (double)d0, acc);
    acc = __builtin_fma((double)d1, (double)d1, acc);
    acc = __builtin_fma((double)d2, (double)d2, acc);
    acc = __builtin_fma((double)d3, (double)d3, acc);
}

// grid (tile pair, slab); scratch[(slab * n + i) * n + j] for the pairs i < j of the tile pair
__global__ __launch_bounds__(256) void fc_pairwise_partial_kernel(const float *pop_slab, int n, int D, int n_slabs,
                                                                   double *scratch)
{
    __shared__ float4 sh[2 * PW_TILE][PW_ROW / 4];
    const int stride = (int)fc_stride(D), P = (int)fc_params(D), g1 = (int)fc_off_g1(D), g2 = (int)fc_off_g2(D);
    const PwBlock B = pw_block(n, stride / PW_CHUNK, n_slabs);
    const int i0 = B.i0, j0 = B.j0, c_lo = B.c_lo, c_hi = B.c_hi, slab = B.slab;
    const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;
    double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0;   // (ti, tj), (ti, tj + 16), (ti + 16, tj), (ti + 16, tj + 16)
    float4 next[4];
    if (c_lo < c_hi) pw_load(pop_slab, n, stride, P, g1, g2, i0, j0, c_lo * PW_CHUNK, next);
    for (int c = c_lo; c < c_hi; ++c) {
        __syncthreads();   // the previous piece has been read by every wave
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int f = (int)threadIdx.x + 256 * m;
            sh[f >> 4][f & 15] = next[m];
        }
        __syncthreads();
        if (c + 1 < c_hi) pw_load(pop_slab, n, stride, P, g1, g2, i0, j0, (c + 1) * PW_CHUNK, next);
#pragma unroll 4
        for (int k = 0; k < PW_CHUNK / 4; ++k) {
            const float4 a0 = sh[ti][k], a1 = sh[ti + 16][k];
            const float4 b0 = sh[PW_TILE + tj][k], b1 = sh[PW_TILE + tj + 16][k];
            pw_fma4(a0, b0, acc00);
            pw_fma4(a0, b1, acc01);
            pw_fma4(a1, b0, acc10);
            pw_fma4(a1, b1, acc11);
        }
    }
    const double acc[2][2] = {{acc00, acc01}, {acc10, acc11}};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i = i0 + ti + 16 * a, j = j0 + tj + 16 * b;
            if (i < n && j < n && i < j) scratch[((size_t)slab * n + i) * n + j] = acc[a][b];
        }
}

// dist[i][j] = dist[j][i] = (float)sqrt(partials of the pair (min, max) added in slab order from +0.0); the diagonal +0.0
__global__ __launch_bounds__(256) void fc_pairwise_finish_kernel(const double *scratch, int n, int n_slabs, float *dist)
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
    dist[idx] = (float)sqrt(tot);
}

// one workgroup per individual: sharing_score_kernel's arithmetic (sharing_row_total) on row blockIdx.x
__global__ __launch_bounds__(256) void niche_counts_kernel(const float *dist, int n, float *niche)
{
    __shared__ double scratch[4];
    const float *row = dist + (size_t)blockIdx.x * n;
    const double tot = sharing_row_total([&](int j) { return row[j]; }, n, scratch);
    if (threadIdx.x == 0) niche[blockIdx.x] = (float)tot;
}

__global__ void ga_fitness_shared_kernel(const double *rewards, int game_first, int pop, int games_per_individual, int hof,
                                         int slot, int flags, const float *share, float *fitness)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pop) return;
    const int gpi = games_per_individual;
    const double *r = rewards + 3 * (size_t)(game_first + i * gpi) + slot;
    double num;
    if (flags & COEVO_FIT_HOF_MEAN) {
        num = 0.0;
        for (int k = 0; k < gpi; ++k) num = num + r[3 * (size_t)k];
    } else {
        num = r[3 * (size_t)(gpi - 1)];   // quirk Q2
    }
    fitness[i] = ga_fitness_value(num, hof, share[(flags & COEVO_FIT_PER_INDIVIDUAL) ? i : 0]);
}

static bool pw_shape_ok(int n, int D) { return n >= 1 && n <= COEVO_SHARING_MAX_POP && fc_dim_ok(D); }

}  // namespace coevo

using namespace coevo;

extern "C" int64_t coevo_fc_pairwise_scratch_doubles(int n, int D)
{
    if (!pw_shape_ok(n, D)) return -1;
    return (int64_t)pw_slabs(n, D) * n * n;
}

extern "C" int coevo_fc_pairwise_distance(const float *pop_slab, int n, int D, double *scratch, float *dist, void *stream)
{
    if (!pop_slab || !scratch || !dist || !pw_shape_ok(n, D) || !aligned16(pop_slab) ||
        (reinterpret_cast<uintptr_t>(scratch) & 7u))
        return COEVO_ERR_ARG;
    const int n_slabs = pw_slabs(n, D);
    hipLaunchKernelGGL(fc_pairwise_partial_kernel, dim3(pw_tile_pairs(n), n_slabs), dim3(256), 0, (hipStream_t)stream, pop_slab,
                       n, D, n_slabs, scratch);
    COEVO_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(fc_pairwise_finish_kernel, dim3((unsigned)(((int64_t)n * n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, scratch, n, n_slabs, dist);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_niche_counts(const float *dist, int n, float *niche, void *stream)
{
    if (!dist || !niche || n < 1 || n > COEVO_SHARING_MAX_POP) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(niche_counts_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, dist, n, niche);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_ga_fitness_shared(const double *rewards, int game_first, int pop, int games_per_individual, int hof,
                                       int slot, int flags, const float *share, float *fitness, void *stream)
{
    if (!rewards || !share || !fitness || pop <= 0 || hof <= 0 || games_per_individual <= 0 || slot < 0 || slot > 2 ||
        game_first < 0 || (flags & ~(COEVO_FIT_HOF_MEAN | COEVO_FIT_PER_INDIVIDUAL)) ||
        (int64_t)game_first + (int64_t)pop * games_per_individual > INT32_MAX)
        return COEVO_ERR_ARG;
    hipLaunchKernelGGL(ga_fitness_shared_kernel, dim3((pop + 127) / 128), dim3(128), 0, (hipStream_t)stream, rewards, game_first,
                       pop, games_per_individual, hof, slot, flags, share, fitness);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
