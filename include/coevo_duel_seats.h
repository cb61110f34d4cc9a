/* libcoevo.so: scripted seats of the paddle duel - env-step entry points in which one parity of every game is played by a
 * scripted seat INSIDE the launch that books the other parity's net (coevonet_amd/duel_crossplay.py).  Like coevo_duel.h it
 * stands beside the pinned ABI of coevo.h (COEVO_VERSION 103): prototypes and constants only, no struct, no name another header
 * declares.  Plain C99; the same library exports these names.  coevonet_amd/lib.py reads this header with the reader of coevo.h
 * into a table of its own.  The rules of the game, the state words and the credit flag are coevo_duel.h's.
 *
 * THE SEAT TABLE: seats [n_games][COEVO_DUEL_SEAT_WORDS] int32, one row per game: {kind, arg, seed low word, seed high word}.
 *   kind COEVO_BL_RANDOM (0), COEVO_BL_PERIODIC (1), COEVO_BL_CONSTANT (2): scripted_action(kind, arg, seed, ordinal, slot, k,
 *     n_actions) of coevo_baseline.h with slot = the seat's parity, k = the number of actions the seat has taken in this game
 *     and ordinal = the game's reset ordinal.
 *   kind COEVO_DUEL_SEAT_TRACKER (3): the seat of player s = its parity reads the newest snapshot (state word 15) alone:
 *     X = 4 for s = 0, 78 for s = 1; p = that player's paddle byte; bx, by = the ball bytes;
 *     top = min(p, by) when bx <= X <= bx + 1 and by + 1 >= p and by <= p + 11 (the ball covers part of the paddle in the
 *     column the tracker reads), else top = p;  d = 2 by + 2 - (2 top + 12);  action 0 if |d| <= 4, 2 if d < 0, else 3 -
 *     whatever n_actions is (an action word >= n_actions moves nothing).  It is atari_duel.duel_tracker_action on the frame.
 *   An invalid seat - a kind outside 0 .. 3, a periodic arg < 0, a constant arg outside 0 .. n_actions - 1 - plays action 0 and
 *   raises COEVO_ST_BAD_TASK in *status.
 *
 * ONE CALL, with t & 1 == script_parity, does per game g, in this order:
 *   1. what coevo_duel_step at t does to the state and acc: t == 0 resets; t >= 1 books the net's action
 *      actions_prev[row_prev[g]] of step t - 1 while t - 1 < limit[g] and the game has not ended;
 *   2. while t < limit[g] and the game has not ended: the seat's action on the state as it now stands, with
 *      k = (t - script_parity) / 2, is stored in script_actions[g] ([n_games] int32; the word is left alone otherwise) and
 *      booked exactly as coevo_duel_step at t + 1 would book it;
 *   3. while t + 1 < limit[g] and the game has not ended: every byte of the frame of step t + 1 (observer (t + 1) & 1) is
 *      written at frames[row_next[g]] (frames == NULL: bookkeeping only).
 * State words, acc and frame bytes are those of coevo_duel_step(t) without frames followed by coevo_duel_step(t + 1) handed the
 * seat's action.  A negative ordinal disables the game as there.
 * COEVO_ERR_ARG, nothing launched: whatever coevo_duel_step refuses (row_next in the place of row_cur), seats, script_actions or
 * status NULL, script_parity outside 0 .. 1, (t & 1) != script_parity.  One launch of n_games workgroups of COEVO_DUEL_THREADS
 * threads on `stream`; synchronises with nothing, allocates nothing, no atomics. */
#ifndef COEVO_DUEL_SEATS_H
#define COEVO_DUEL_SEATS_H
#include "coevo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COEVO_DUEL_SEAT_WORDS 4
#define COEVO_DUEL_SEAT_TRACKER 3

int coevo_duel_seat_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0, const int32_t *gen_dev,
                         int64_t ordinals_per_gen, int t, const int32_t *limit, const int32_t *seats, int script_parity,
                         const int32_t *row_prev, const int32_t *actions_prev, int32_t *script_actions, const int32_t *row_next,
                         uint8_t *frames, int C, int n_actions, uint64_t seed, int points_to_win, int flags, int32_t *status,
                         void *stream);

/* coevo_duel_seat_step for t >= 1 with the float32 output layer of the net's step t - 1 in the same launch, as
 * coevo_dqn_out_duel_step carries it: the same added arguments and the same single exception - the row of a finished game
 * (t - 1 >= limit, ended by points, or disabled) is not evaluated, its actions_prev word keeps what it held and raises nothing.
 * Also COEVO_ERR_ARG: t < 1, slab, tasks_prev or workspace NULL, n_tasks_prev <= 0, n_rows_total <= 0. */
int coevo_dqn_out_duel_seat_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0,
                                 const int32_t *gen_dev, int64_t ordinals_per_gen, int t, const int32_t *limit,
                                 const int32_t *seats, int script_parity, const int32_t *row_prev, int32_t *actions_prev,
                                 int32_t *script_actions, const int32_t *row_next, uint8_t *frames, int C, int n_actions,
                                 uint64_t seed, int points_to_win, int flags, const float *slab,
                                 const coevo_dqn_task *tasks_prev, int n_tasks_prev, int n_rows_total, const void *workspace,
                                 int32_t *status, void *stream);

/* ... over an fp16 slab, with the extra rules of coevo_dqn16_out_duel_step: the float16 output row, the same exception, a task
 * the float16 forward cannot serve gets no output row (the action booked is the word actions_prev already holds), and a slab
 * that is not 16-byte aligned is COEVO_ERR_ARG. */
int coevo_dqn16_out_duel_seat_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0,
                                   const int32_t *gen_dev, int64_t ordinals_per_gen, int t, const int32_t *limit,
                                   const int32_t *seats, int script_parity, const int32_t *row_prev, int32_t *actions_prev,
                                   int32_t *script_actions, const int32_t *row_next, uint8_t *frames, int C, int n_actions,
                                   uint64_t seed, int points_to_win, int flags, const void *slab,
                                   const coevo_dqn_task *tasks_prev, int n_tasks_prev, int n_rows_total, const void *workspace,
                                   int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
