// coevo_crossplay_reduce (include/coevo_crossplay.h): the per-game reward triples of a cross-play rollout -> the payoff table
// [A][B][C][3] and its three marginals, in main.py's order (`total += reward` from 0.0, one division; population.mean_eval).
//
// The order is the contract, so every output word is ONE thread's sequential fp64 chain: no tree, no atomics, no partial sums
// handed between workgroups.  The work is tiny beside the rollout that produced the rewards (3 n doubles read once for the
// payoffs, 9 A B C doubles for the marginals), so the chains are left as they are rather than made fast in another order.
#include "coevo_common.hip.h"

#include "../../include/coevo_crossplay.h"

namespace coevo {

// thread i = 3 t + s: payoff[t][s] over the E games of trio t
__global__ void crossplay_payoff_kernel(const double *rewards, int n_trios, int E, double *payoff)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (3 n_trios + 127 can leave int32: 64-bit indices)
    if (i >= 3 * (int64_t)n_trios) return;
    const int64_t t = i / 3, s = i % 3;
    const double *r = rewards + (size_t)t * E * 3 + s;
    double tot = 0.0;
    for (int e = 0; e < E; ++e) tot = tot + r[3 * (size_t)e];
    payoff[i] = tot / (double)E;
}

// thread i over [marg_a | marg_b | marg_c] words (a missing table takes no threads): net j of its role, slot s; the trios that
// seat it in ascending t = (a B + b) C + c - the two other indices in row-major order
__global__ void crossplay_marginal_kernel(const double *payoff, int A, int B, int C, double *marg_a, double *marg_b, double *marg_c)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t na = marg_a ? 3 * (int64_t)A : 0, nb = marg_b ? 3 * (int64_t)B : 0, nc = marg_c ? 3 * (int64_t)C : 0;
    if (i >= na + nb + nc) return;
    double tot = 0.0;
    if (i < na) {
        const int64_t a = i / 3, s = i % 3;
        const double *p = payoff + (size_t)a * B * C * 3 + s;
        for (int k = 0; k < B * C; ++k) tot = tot + p[3 * (size_t)k];
        marg_a[i] = tot / (double)(B * C);
        return;
    }
    i -= na;
    if (i < nb) {
        const int64_t b = i / 3, s = i % 3;
        for (int a = 0; a < A; ++a) {
            const double *p = payoff + ((size_t)a * B + b) * C * 3 + s;
            for (int c = 0; c < C; ++c) tot = tot + p[3 * (size_t)c];
        }
        marg_b[i] = tot / (double)(A * C);
        return;
    }
    i -= nb;
    const int64_t c = i / 3, s = i % 3;
    for (int ab = 0; ab < A * B; ++ab) tot = tot + payoff[((size_t)ab * C + c) * 3 + s];
    marg_c[i] = tot / (double)(A * B);
}

static bool words_overlap(const double *a, size_t na, const double *b, size_t nb)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + 8 * nb && b0 < a0 + 8 * na;
}

}  // namespace coevo

extern "C" int coevo_crossplay_reduce(const double *rewards, int A, int B, int C, int E, double *payoff, double *marg_a,
                                      double *marg_b, double *marg_c, void *stream)
{
    if (!rewards || !payoff || A <= 0 || B <= 0 || C <= 0 || E <= 0) return COEVO_ERR_ARG;
    const int64_t max_games = INT32_MAX / 3;
    int64_t n = A;   // every partial product is checked, so none leaves int64
    const int dims[3] = {B, C, E};
    for (int d : dims) {
        n *= d;
        if (n > max_games) return COEVO_ERR_ARG;
    }
    const int n_trios = A * B * C;
    const size_t n_words = 3 * (size_t)n;
    double *const outs[4] = {payoff, marg_a, marg_b, marg_c};
    const size_t out_words[4] = {3 * (size_t)n_trios, 3 * (size_t)A, 3 * (size_t)B, 3 * (size_t)C};
    for (int k = 0; k < 4; ++k)
        if (outs[k] && coevo::words_overlap(rewards, n_words, outs[k], out_words[k])) return COEVO_ERR_ARG;
    hipLaunchKernelGGL(coevo::crossplay_payoff_kernel, dim3((unsigned)((3 * (int64_t)n_trios + 127) / 128)), dim3(128), 0,
                       (hipStream_t)stream, rewards, n_trios, E, payoff);
    COEVO_HIP_CHECK(hipGetLastError());
    const int64_t n_marg = (marg_a ? 3 * (int64_t)A : 0) + (marg_b ? 3 * (int64_t)B : 0) + (marg_c ? 3 * (int64_t)C : 0);
    if (n_marg == 0) return COEVO_OK;
    hipLaunchKernelGGL(coevo::crossplay_marginal_kernel, dim3((unsigned)((n_marg + 127) / 128)), dim3(128), 0, (hipStream_t)stream,
                       payoff, A, B, C, marg_a, marg_b, marg_c);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}
