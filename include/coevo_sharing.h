/* libcoevo.so: population-sharing surface - the entry points behind GAEngine(hof_mean=..., population_sharing=...), the two
 * Co-GA extension modes that are NOT the reference's algorithm: fitness over every Hall-of-Fame game, and fitness
 * sharing by a per-individual niche count over all pairwise distances of the population.  Like coevo_ext.h and
 * coevo_crossplay.h it stands beside the pinned ABI of coevo.h (COEVO_VERSION 103): prototypes and constants only, no struct,
 * no name the three other headers declare.  Plain C99; the same library exports these names.  coevonet_amd/lib.py reads this
 * header with the reader of coevo.h into a table of its own. */
#ifndef COEVO_SHARING_H
#define COEVO_SHARING_H
#include "coevo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COEVO_SHARING_MAX_POP 4096          /* coevo_rank_desc's limit */
#define COEVO_FIT_HOF_MEAN 1                /* flags of coevo_ga_fitness_shared */
#define COEVO_FIT_PER_INDIVIDUAL 2

/* Doubles of scratch that coevo_fc_pairwise_distance needs for n nets of observation width D: slabs(n) * n * n, where slabs(n)
 * (<= 64) is the number of pieces the parameter axis is cut into.  < 0: n outside 1 .. COEVO_SHARING_MAX_POP or D not 8 / 10. */
int64_t coevo_fc_pairwise_scratch_doubles(int n, int D);

/* All pairwise distances of the n nets at pop_slab (coevo_fc_slab_stride(D) floats apart), in fc_distance_kernel's arithmetic:
 *   dist[i][j] = (float)sqrt(sum_p (double)df * (double)df),  df = w_j[p] - w_i[p] in fp32,
 * p over the Linear weights and biases only (LayerNorm gamma / beta and the stride's padding never count, whatever they hold).
 * The squares are exact in fp64; the fp64 sum runs in an order that is fixed for given (n, D) - no floating-point atomics, two
 * runs give the same words.  dist[i][j] and dist[j][i] are the same bits, dist[i][i] is +0.0 (also for a net with inf or NaN
 * entries, whose other distances are inf or NaN).  Every word of dist [n][n] is written; scratch
 * [coevo_fc_pairwise_scratch_doubles(n, D)] may hold anything before and holds the partial sums after.  Two launches on
 * `stream`.  COEVO_ERR_ARG, nothing launched: a NULL pointer, n outside 1 .. COEVO_SHARING_MAX_POP, D not 8 / 10, pop_slab not
 * 16-byte aligned, scratch not 8-byte aligned. */
int coevo_fc_pairwise_distance(const float *pop_slab, int n, int D, double *scratch, float *dist, void *stream);

/* niche[i] = coevo_sharing_score's arithmetic on row i of dist [n][n], the self term dist[i][i] included (the reference's
 * diversity_penalty is handed the population list, which holds the individual):
 *   sigma_i = (float)(sum_j (double)dist[i][j] / n);  sh = 1.0f - dist[i][j] / sigma_i;  niche[i] = (float)sum (double)sh over
 *   the j where !(sh <= 0)
 * so a population of identical nets gives NaN everywhere.  One launch, one workgroup per row.  COEVO_ERR_ARG: a NULL pointer,
 * n outside 1 .. COEVO_SHARING_MAX_POP. */
int coevo_niche_counts(const float *dist, int n, float *niche, void *stream);

/* coevo_ga_fitness with two switches.  Individual i's games are rewards[game_first + i * games_per_individual + k][slot],
 * k < games_per_individual:
 *   COEVO_FIT_HOF_MEAN        total = (float)((+0.0 + r_0 + r_1 + ...) / (double)hof), k ascending in fp64; without it the last
 *                             game alone, (float)(r_last / (double)hof) (quirk Q2)
 *   COEVO_FIT_PER_INDIVIDUAL  fitness[i] = total / (1.0f + share[i]), share [pop]; without it share is one word, share[0]
 * flags 0 is coevo_ga_fitness bit for bit.  COEVO_ERR_ARG: what coevo_ga_fitness refuses, flags outside 0 .. 3, or
 * game_first + pop * games_per_individual above INT32_MAX. */
int coevo_ga_fitness_shared(const double *rewards, int game_first, int pop, int games_per_individual, int hof, int slot,
                            int flags, const float *share, float *fitness, void *stream);

#ifdef __cplusplus
}
#endif
#endif
