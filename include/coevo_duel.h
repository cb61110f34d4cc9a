/* libcoevo.so: paddle-duel surface - the env-step entry points behind coevonet_amd/atari_duel.py (a two-player ball game WITH
 * dynamics in the AEC shape of pettingzoo.atari, for the DeepQN engines; it is not ALE Pong and does not claim to be).  Like
 * coevo_gauntlet.h it stands beside the pinned ABI of coevo.h (COEVO_VERSION 103): prototypes and constants only, no struct, no
 * name another header declares.  Plain C99; the same library exports these names.  coevonet_amd/lib.py reads this header with the
 * reader of coevo.h into a table of its own.
 *
 * THE RULES (all arithmetic is integer; coevonet_amd/atari_duel.py states the same in plain Python)
 * Field: 84 x 84 pixels, frame[y][x][c] uint8 in HWC order, byte (84 y + x) C + c.  Paddle of first_0: columns 4-5, rows
 * p0 .. p0 + 11; paddle of second_0: columns 78-79, rows p1 .. p1 + 11; p in [0, 72].  Ball: 2 x 2 at top-left (bx, by), both in
 * [0, 82].  Velocity: vx in {-3, +3}, vy in [-3, 3].
 * Action -> paddle move: MOVE[a mod 6] = (0, 0, -4, +4, -4, +4) for 0 <= a < n_actions, any other action word moves nothing;
 * p = clamp(p + move, 0, 72).
 * AEC order: first_0 acts at even agent-steps (its action is only stored), second_0 at odd ones; the world then steps once:
 *   1. both paddles move;  2. bx += vx, by += vy;
 *   3. wall: by < 0 -> by = -by, vy = -vy;  by > 82 -> by = 164 - by, vy = -vy;
 *   4. left plane, when vx < 0 and bx <= 5: off = by + 1 - p0; 0 <= off <= 12 is a hit: bx = 12 - bx, vx = +3, vy = VY[off],
 *      VY = (-3,-2,-2,-1,-1,0,0,0,1,1,2,2,3); otherwise a point for second_0: r = (-1, +1);
 *   5. right plane, when vx > 0 and bx >= 77: off = by + 1 - p1; a hit gives bx = 152 - bx, vx = -3, vy = VY[off]; a miss
 *      r = (+1, -1);
 *   6. after a point: a score that has reached points_to_win ends the game; otherwise serve number k = score0 + score1 (the
 *      paddles stay);
 *   7. the snapshot bx | by << 8 | p0 << 16 | p1 << 24 (low bytes) enters the four-deep history.
 * Serve k of the game with reset ordinal o under seed s: w = philox4x32_10(counter (0xFFFFFFFE, k, low word of o, high word of
 * o ^ 0x73657276), key (low word of s, high word of s)); bx = 41, by = 8 + w[2] mod 68, vx = w[0] & 1 ? +3 : -3,
 * vy = (-2, -1, 1, 2)[w[1] & 3].  Reset = serve 0 with p0 = p1 = 36, scores 0, no pending action, four equal snapshots.
 * Observation: planes 0 .. 3 are the four snapshots rendered, oldest first (ball 255, paddles 160, background 0, the ball on
 * top); C == 6 adds plane 4 = 255 for the observer first_0 and plane 5 = 255 for the observer second_0.
 * Books: PettingZoo's (the actor's cumulative reward is zeroed when it steps; a world step adds r to both).  Credit "next"
 * (flags 0) is play_atari's quirk: the actor receives the cumulative reward of the agent that acts NEXT, read after its step -
 * first_0 at even t cum1, second_0 at odd t cum0 after the world step.  The game is zero-sum, so "next" rewards losing: the
 * reference's rule.  COEVO_DUEL_CREDIT_OWN credits the actor with its own reward of the latest world step instead (second_0 in
 * the step that moved the world, first_0 when it steps next): the negation of "next", step for step.
 * A game that has ended books nothing further and renders nothing further. */
#ifndef COEVO_DUEL_H
#define COEVO_DUEL_H
#include "coevo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* int32 words of one game's state:
 *   0        the pending action of first_0 (COEVO_DUEL_NO_ACTION: none)
 *   1 .. 6   bx, by, vx, vy, p0, p1
 *   7 .. 10  score0, score1, cum0, cum1
 *   11       ended: 0 while the game runs, else the count of agent-steps it had booked when it ended
 *   12 .. 15 the four history snapshots, oldest first */
#define COEVO_DUEL_STATE_WORDS 16
#define COEVO_DUEL_NO_ACTION 0xFF
#define COEVO_DUEL_CREDIT_OWN 1   /* flags bit 0 */
#define COEVO_DUEL_THREADS 256    /* one workgroup of this many threads per game */

/* coevo_synth_step's argument meaning over the duel.  One call = the env side of agent-step t for every game g of 0 ..
 * n_games - 1: t == 0 resets the state and acc[g][0 .. 2]; t >= 1 books the action of step t - 1, actions_prev[row_prev[g]], of
 * actor (t - 1) & 1, while t - 1 < limit[g] and the game has not ended; then, while t < limit[g] and the game has not ended, every
 * byte of the frame of step t (observer t & 1) is written at frames[row_cur[g]] (frames == NULL: bookkeeping only).
 * ordinal(g) = game_ordinal0[g] + *gen_dev * ordinals_per_gen (gen_dev may be NULL); a negative ordinal disables the game:
 * nothing of it is booked or rendered (t == 0 still resets its words).
 *   duel_state [n_games][COEVO_DUEL_STATE_WORDS] int32, acc [n_games][3] fp64 = play_game's (first_0, second_0) returns + one
 *   unused slot, limit [n_games], frames [rows][84][84][C] uint8, 16-byte aligned: device memory.
 * COEVO_ERR_ARG, nothing launched: duel_state, acc, game_ordinal0 or limit NULL, n_games <= 0, t outside 0 .. 65535, C not 4 or
 * 6, n_actions outside 1 .. COEVO_DQN_LOGIT_STRIDE, points_to_win < 1, a flags bit other than COEVO_DUEL_CREDIT_OWN, row_prev or
 * actions_prev NULL with t > 0, row_cur NULL with frames, frames not 16-byte aligned.  One launch on `stream`; synchronises with
 * nothing and allocates nothing. */
int coevo_duel_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0, const int32_t *gen_dev,
                    int64_t ordinals_per_gen, int t, const int32_t *limit, const int32_t *row_prev, const int32_t *actions_prev,
                    const int32_t *row_cur, uint8_t *frames, int C, int n_actions, uint64_t seed, int points_to_win, int flags,
                    void *stream);

/* coevo_duel_step for t >= 1 with the output layer of step t - 1 in the same launch, exactly as coevo_dqn_out_synth_step carries
 * it: game g's workgroup turns the hidden row row_prev[g] of the workspace coevo_dqn_forward_hidden_timed filled into logits and
 * the first-max action, stores it in actions_prev, books it and renders.  Same effects as coevo_dqn_forward_argmax +
 * coevo_duel_step with ONE exception: the row of a finished game (t - 1 >= limit, ended by points, or disabled) is not
 * evaluated - its actions_prev word keeps what it held and raises nothing.  COEVO_ERR_ARG (nothing launched): as
 * coevo_duel_step, t < 1, slab, tasks_prev, workspace or status NULL, n_tasks_prev <= 0, n_rows_total <= 0. */
int coevo_dqn_out_duel_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0, const int32_t *gen_dev,
                            int64_t ordinals_per_gen, int t, const int32_t *limit, const int32_t *row_prev, int32_t *actions_prev,
                            const int32_t *row_cur, uint8_t *frames, int C, int n_actions, uint64_t seed, int points_to_win,
                            int flags, const float *slab, const coevo_dqn_task *tasks_prev, int n_tasks_prev, int n_rows_total,
                            const void *workspace, int32_t *status, void *stream);

/* ... over an fp16 slab (coevo_dqn16_pack's layout, 16-byte aligned; the workspace of coevo_dqn16_forward_hidden), as
 * coevo_dqn16_out_synth_step: the float16 output row, the same exception, and a task the float16 forward cannot serve gets no
 * output row - the action booked is the word actions_prev already holds.  Also COEVO_ERR_ARG: a slab not 16-byte aligned. */
int coevo_dqn16_out_duel_step(int32_t *duel_state, double *acc, int n_games, const int64_t *game_ordinal0,
                              const int32_t *gen_dev, int64_t ordinals_per_gen, int t, const int32_t *limit,
                              const int32_t *row_prev, int32_t *actions_prev, const int32_t *row_cur, uint8_t *frames, int C,
                              int n_actions, uint64_t seed, int points_to_win, int flags, const void *slab,
                              const coevo_dqn_task *tasks_prev, int n_tasks_prev, int n_rows_total, const void *workspace,
                              int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
