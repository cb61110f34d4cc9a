/* libcoevo.so: baseline-gauntlet surface - the entry points behind coevonet_amd/gauntlet.py (a few dozen simple_adversary games
 * of evolved nets against baseline seats, every env-cycle of every game in ONE launch).  Like coevo_baseline.h it stands beside
 * the pinned ABI of coevo.h (COEVO_VERSION 103): prototypes and constants only, no struct, no name another header declares.
 * Plain C99; the same library exports these names.  coevonet_amd/lib.py reads this header with the reader of coevo.h into a table
 * of its own. */
#ifndef COEVO_GAUNTLET_H
#define COEVO_GAUNTLET_H
#include "coevo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Seat kinds of a gauntlet game: COEVO_BL_RANDOM / _PERIODIC / _CONSTANT (0, 1, 2) of coevo_baseline.h and */
#define COEVO_GT_FC 3    /* an evolved FCNetwork in the fc slab layout (coevo_fc_pack) */
#define COEVO_GT_MLP 4   /* a PPO policy net in flat order (coevo_baseline.h) */
/* int32 words per game.  Env slot s (0 adversary_0, 1 agent_0, 2 agent_1) owns words 4 s .. 4 s + 3 =
 *   {kind, arg, seed low word, seed high word}
 * arg: the net's float offset into `slab` (COEVO_GT_FC) or into `mlp_nets` (COEVO_GT_MLP), the start (COEVO_BL_PERIODIC), the
 * action (COEVO_BL_CONSTANT); the seed words are read by COEVO_BL_RANDOM only.  Words 12 .. 15 are zero.  The width of a net
 * follows from its slot: 8 for slot 0, 10 for slots 1 and 2. */
#define COEVO_GT_GAME_WORDS 16
#define COEVO_GT_THREADS 256   /* one workgroup of this many threads per game */
#define COEVO_GT_WAVE_ROWS 4   /* coevo_mlp_forward_argmax_wave: rows a workgroup serves per pass, one per wave */

/* For every game g of 0 .. n_games - 1 and every cycle c = cycle_first .. cycle_first + n_cycles - 1, in this order:
 *   1. obs_scratch[3 g + s][0 .. COEVO_OBS_STRIDE) = the observation of slot s, coevo_mpe_observe's values (zeros behind the width)
 *   2. actions[3 g + s] = the seat's action: COEVO_GT_FC the canonical FCNetwork forward and first maximum
 *      (coevo_fc_forward_argmax's), COEVO_GT_MLP the policy-net contract of coevo_baseline.h (a faulted row plays 0), a scripted
 *      kind scripted_action(kind, arg, seed, (uint64_t)game_ordinal[g] + ordinal_add, s, c, 5)
 *   3. the world cycle of coevo_mpe_step(state, n_games, rows 3 g + s, actions, c, game_limit, pos_first) for game g
 * - the launches of one env-cycle of coevonet_amd.baselines.BaselineCrossPlay, for one game, in one workgroup.  Numerical faults
 * are or-ed into *status as those launches raise them (COEVO_ST_BAD_INPUT .. COEVO_ST_NO_ACTION).  A game with a bad word - a
 * kind outside 0 .. 4, a net offset that is negative, not a multiple of 4 floats or whose net leaves 0 .. slab_floats /
 * 0 .. mlp_floats, a constant outside 0 .. 4, a periodic start below 0 - is skipped with COEVO_ST_BAD_TASK: its state, its
 * observation rows and its actions are not touched and nothing is read through its words.
 * slab [slab_floats], mlp_nets [mlp_floats] (may be NULL when mlp_floats == 0), games [n_games][COEVO_GT_GAME_WORDS],
 * game_ordinal [n_games], state [COEVO_MPE_STATE_DOUBLES][n_games], game_limit [n_games], obs_scratch
 * [3 n_games][COEVO_OBS_STRIDE], actions [3 n_games], status [1]: device memory.  No workgroup waits for another.
 * COEVO_ERR_ARG, nothing launched: slab, games, game_ordinal, state, game_limit, obs_scratch, actions or status NULL, mlp_nets
 * NULL with mlp_floats != 0, slab or mlp_nets not 16-byte aligned, slab_floats < 0, mlp_floats < 0, n_games < 0, cycle_first < 0,
 * n_cycles < 0, cycle_first + n_cycles above INT32_MAX / 3.  n_games == 0 or n_cycles == 0 is COEVO_OK without a launch.  One launch on `stream`;
 * synchronises with nothing and allocates nothing. */
int coevo_mpe_gauntlet(const float *slab, int64_t slab_floats, const float *mlp_nets, int64_t mlp_floats, const int32_t *games,
                       int n_games, const int64_t *game_ordinal, uint64_t ordinal_add, double *state, const int32_t *game_limit,
                       int cycle_first, int n_cycles, int pos_first, float *obs_scratch, int32_t *actions, int32_t *status,
                       void *stream);

/* coevo_mlp_forward_argmax (coevo_baseline.h: same arguments, task words, refusals, outputs and bits) with one WAVE per row:
 * lane j owns hidden unit j of both layers, lanes 0 .. 4 the logits; every output is still its one sequential fmaf chain over k
 * ascending from the bias.  A workgroup serves its task's rows COEVO_GT_WAVE_ROWS at a time.  The form of a launch with few
 * rows: the dependent chain of a row is D + 64 + 64 steps, not 5 056. */
int coevo_mlp_forward_argmax_wave(const float *nets, int64_t nets_floats, const int32_t *tasks, int n_tasks, const float *obs,
                                  int n_rows, int32_t *actions, float *logits, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
