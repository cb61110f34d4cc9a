/* libcoevo.so: baseline-opponent surface - the entry points behind coevonet_amd/baselines.py (cross-play against seats that
 * are not evolved nets: scripted policies and small PPO policy nets).  Like coevo_crossplay.h it stands beside the pinned ABI
 * of coevo.h (COEVO_VERSION 103): prototypes and constants only, no struct, no name another header declares.  Plain C99; the
 * same library exports these names.  coevonet_amd/lib.py reads this header with the reader of coevo.h into a table of its own. */
#ifndef COEVO_BASELINE_H
#define COEVO_BASELINE_H
#include "coevo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- scripted seats ------------------------------------- */
/* scripted_action(kind, arg, seed, ordinal, slot, k, n_actions) - one statement, here and in coevonet_amd/baselines.py:
 *   COEVO_BL_RANDOM    w = philox4x32_10(ordinal & 0xffffffff, ordinal >> 32, k, slot, seed & 0xffffffff, seed >> 32)[0]
 *                      (the ten-round generator of the synthetic env), action = (w * n_actions) >> 32 in 64 bits
 *   COEVO_BL_PERIODIC  (arg + k) % n_actions, arg >= 0, the sum in 64 bits
 *   COEVO_BL_CONSTANT  arg, 0 <= arg < n_actions
 * k = how many actions the seat has taken in this game, ordinal = the game's reset ordinal, slot = the env slot of the seat
 * (0 adversary_0, 1 agent_0, 2 agent_1; the parity for the two-player games).  The action depends on the episode, not on the
 * game's place in the table. */
#define COEVO_BL_RANDOM 0
#define COEVO_BL_PERIODIC 1
#define COEVO_BL_CONSTANT 2
/* int32 words per scripted seat: {game, row, kind, arg, seed low word, seed high word, slot, 0} */
#define COEVO_BL_SEAT_WORDS 8

/* actions[seat.row] = scripted_action(seat.kind, seat.arg, seat.seed, (uint64_t)game_ordinal[seat.game] + ordinal_add, seat.slot,
 * k, n_actions) for the n_seats seats of `seats` (device, [n_seats][COEVO_BL_SEAT_WORDS]); no other word of `actions` is
 * touched.  A seat whose game is outside 0 .. n_games - 1, whose row is outside 0 .. n_rows - 1, whose kind is none of the
 * three, a periodic seat with arg < 0 or a constant outside 0 .. n_actions - 1 writes nothing.  game_ordinal: device
 * [n_games].  COEVO_ERR_ARG, nothing launched: a NULL pointer, n_seats < 0, n_games <= 0, n_rows <= 0, n_actions outside
 * 1 .. 32.  n_seats == 0 is COEVO_OK without a launch.  One launch on `stream`, one thread per seat. */
int coevo_baseline_actions(const int32_t *seats, int n_seats, const int64_t *game_ordinal, uint64_t ordinal_add, int n_games,
                           uint32_t k, int n_actions, int32_t *actions, int n_rows, void *stream);

/* ---------------------------------------------------------------- PPO policy nets ------------------------------------ */
/* The policy of a PPO baseline: D -> 64 -> 64 -> 5, ReLU.  A net is its flat parameter order - fc1.weight [64][D], fc1.bias,
 * fc2.weight [64][64], fc2.bias, policy_head.weight [5][64], policy_head.bias - as it is; nets lie in `nets` at offsets that
 * are multiples of 4 floats (coevo_mlp_slab_stride(D) apart).  Arithmetic (fp32): every output is one sequential fmaf chain
 * over k ascending that starts from the bias, ReLU is v > 0 ? v : +0, the action is the first maximum of a strict > scan over
 * the five logits.  A non-finite observation, fc1 output, fc2 output or logit raises COEVO_ST_BAD_INPUT / _BAD_FC1 / _BAD_FC2
 * / _BAD_OUT in *status (the outputs are checked before the ReLU); such a row plays 0.  Logits are written as computed. */
#define COEVO_MLP_H 64
#define COEVO_MLP_NACT 5
#define COEVO_MLP_ROW_TILE 256   /* rows of one task = of one workgroup, one row per thread */
/* int32 words per task: {net_off (floats into `nets`), first (row / seat), count (1 .. COEVO_MLP_ROW_TILE), D (8 or 10)} */
#define COEVO_MLP_TASK_WORDS 4
/* int32 words per seat: {game, row, slot, 0} */
#define COEVO_MLP_SEAT_WORDS 4
int coevo_mlp_param_count(int D);   /* 5189 (D = 10) / 5061 (D = 8); COEVO_ERR_ARG for another width */
int coevo_mlp_slab_stride(int D);   /* the count rounded up to a multiple of 4 floats */

/* obs [n_rows][COEVO_OBS_STRIDE] -> actions [n_rows], logits [n_rows][COEVO_LOGIT_STRIDE] (or NULL; five floats of a row are
 * written).  Task t serves rows first .. first + count - 1 with the net at net_off.  A task with D not 8 / 10, count outside
 * 1 .. COEVO_MLP_ROW_TILE, rows outside 0 .. n_rows - 1, or a net that is not 4-float aligned or leaves 0 .. nets_floats is
 * skipped with COEVO_ST_BAD_TASK.  COEVO_ERR_ARG, nothing launched: a NULL pointer (but logits), `nets` not 16-byte aligned,
 * n_tasks < 0, n_rows <= 0.  n_tasks == 0 is COEVO_OK without a launch.  One launch on `stream`, one workgroup per task. */
int coevo_mlp_forward_argmax(const float *nets, int64_t nets_floats, const int32_t *tasks, int n_tasks, const float *obs,
                             int n_rows, int32_t *actions, float *logits, int32_t *status, void *stream);

/* observe + forward + first maximum for seats of simple_adversary games: task t serves seats first .. first + count - 1 of
 * `seats` (device, [n_seats][COEVO_MLP_SEAT_WORDS]); seat i observes slot seat.slot of game seat.game (coevo_mpe_observe's
 * values) and writes actions[seat.row]; logits (or NULL) [n_seats][COEVO_LOGIT_STRIDE] by seat.  The width comes from the
 * seat's slot; a seat whose width is not its task's, or whose game / row / slot is out of range, raises COEVO_ST_BAD_TASK and
 * writes nothing.  Otherwise as coevo_mlp_forward_argmax. */
int coevo_mpe_mlp_policy_cycle(const float *nets, int64_t nets_floats, const int32_t *tasks, int n_tasks, const int32_t *seats,
                               int n_seats, const double *state, int n_games, int32_t *actions, int n_rows, float *logits,
                               int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
