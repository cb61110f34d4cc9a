/* libcoevo.so: population sharing over float16 nets - the all-pairs distance behind HalfGAEngine(population_sharing=True), the
 * fp16 twin of coevo_fc_pairwise_distance (coevo_sharing.h).  The niche counts, the fitness with its switches and
 * the ranking are coevo_sharing.h's and coevo.h's entry points on the fp16-valued matrix.  Like coevo_sharing.h it stands beside
 * the pinned ABI of coevo.h: prototypes only, no struct, no name the four other headers declare.  Plain C99; the same library
 * exports these names.  coevonet_amd/lib.py reads this header with the reader of coevo.h into a table of its own. */
#ifndef COEVO_SHARING16_H
#define COEVO_SHARING16_H
#include "coevo_sharing.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Doubles of scratch that coevo_fc16_pairwise_distance needs for n nets of observation width D: slabs(n) * n * n, slabs(n) <= 64
 * pieces of the parameter axis.  < 0: n outside 1 .. COEVO_SHARING_MAX_POP or D not 8 / 10. */
int64_t coevo_fc16_pairwise_scratch_doubles(int n, int D);

/* All pairwise distances of the n nets at pop_slab (fp16 slabs, coevo_fc16_slab_stride(D) words apart), in the float16
 * distance contract of coevo_fc16_distance + coevo_fc16_distance_finalize:
 *   dist[i][j] = f16(sqrt(sum_p (double)d * d)),  d = f16(f32(w_i[p]) - f32(w_j[p])),  the root rounded once to fp16,
 * stored as an fp32 word; p over the Linear entries only - the W2h, W1h and W3h halves and the b1, b2, b3 words, which hold
 * fp16 values (LayerNorm gamma / beta, the stride's padding and nets past n never count, whatever they hold).  The squares
 * are exact; the fp64 sum runs in an order that is fixed for given (n, D) - no floating-point atomics.  dist[i][j] and
 * dist[j][i] are the same bits, dist[i][i] is +0.0 (also for a net with inf entries, whose other distances are inf).  Every
 * word of dist [n][n] is written; scratch [coevo_fc16_pairwise_scratch_doubles(n, D)] may hold anything before and holds the
 * partial sums after.  Two launches on `stream`.  COEVO_ERR_ARG, nothing launched: a NULL pointer, n outside
 * 1 .. COEVO_SHARING_MAX_POP, D not 8 / 10, pop_slab not 16-byte aligned, scratch not 8-byte aligned. */
int coevo_fc16_pairwise_distance(const void *pop_slab, int n, int D, double *scratch, float *dist, void *stream);

#ifdef __cplusplus
}
#endif
#endif
