/* libcoevo.so: extension surface - additions that are not yet part of the pinned ABI of coevo.h (COEVO_VERSION 103: its set of
 * entry points, structs and constants is frozen by tests/test_abi.py and tests/golden/abi_tables.json).  Plain C99; the same
 * library exports these names.  coevonet_amd/lib.py reads this header with the reader of coevo.h into a table of its own.
 * An entry point moves into coevo.h with the next COEVO_VERSION. */
#ifndef COEVO_EXT_H
#define COEVO_EXT_H
#include "coevo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- DeepQN in float16: the TILED fc1 block ------------- */
/* A second form of the fp16 DeepQN slab (coevo_dqn16_pack's; Atari/deepqn.py:12-37).  Sections, offsets and the stride
 * (coevo_dqn16_slab_stride) are the same; the fc1 block - 512 * 3136 halves - is a permutation of its halves:
 *   tiled [out block ob of 64][S = k / 32][T = 16-out tile][lane = 16 (k % 4) + out % 16][j = (k / 4) % 8]
 * The 16-byte piece of lane (c, kk) in (ob, S, T) holds fc1.w[64 ob + 16 T + c][32 S + 4 j + kk], j = 0 .. 7: for tile T the B
 * operands of the eight consecutive v_mfma_f32_16x16x4 k-quads 8 S .. 8 S + 7.  A slab's form is an attribute of its owner: no
 * word of the slab records it, and the tiled form is reached through the names below only.  Each takes the PLAIN channel count
 * 1 .. 6 (COEVO_DQN_FC1_TILED or any other bit or-ed into C is COEVO_ERR_ARG, as for its streamed twin; every coevo_dqn16_* and
 * coevo_dqn_es16_* entry point of coevo.h keeps refusing that bit).  Each takes the arguments of its twin and refuses what
 * the twin refuses, with nothing written.
 * coevo_dqn16_distance and coevo_fc16_distance_finalize serve tiled slabs UNCHANGED when both nets have one form: the block is a
 * permutation and every 16-byte piece holds eight halves, so the same terms d = f16(f32(a) - f32(b)) are summed in fp64, in a
 * fixed (other) order.  coevo_dqn16_out_synth_step never reads fc1 and serves both forms. */
#define COEVO_DQN16_FC1_SUPER 98   /* super-pieces S (32 k) per output block */

/* coevo_dqn16_pack / coevo_dqn16_unpack straight to and from the tiled form (AtariAgent weights <-> slab; pack rounds every
 * entry to fp16 to nearest even and zeroes the stride's padding) */
int coevo_dqn16_pack_tiled(const float *flat, void *slab, int n, int C, int n_actions, void *stream);
int coevo_dqn16_unpack_tiled(const void *slab, float *flat, int n, int C, int n_actions, void *stream);
/* n nets of src (fc1 form src_tiled: 0 streamed, 1 tiled) into dst (form dst_tiled): the fc1 block's halves move to their places
 * in the other form (equal flags: a copy), every other word of the stride - its padding included - is copied as it is.
 * COEVO_ERR_ARG, with nothing written: a NULL pointer, src == dst, a pointer that is not 16-byte aligned, n < 0, a bad shape, a flag
 * other than 0 / 1.  n == 0 is COEVO_OK.  The nets must not overlap.  One launch on `stream`. */
int coevo_dqn16_relayout(const void *src, void *dst, int n, int C, int n_actions, int src_tiled, int dst_tiled, void *stream);

/* coevo_dqn16_forward_hidden / coevo_dqn16_forward_argmax (the half modules of Atari/deepqn.py:12-37) over a slab whose fc1 block is tiled: the same conv-stack and output launches, fc1 by dqn16_fc1_tiled_kernel - one wave per (task, 64-output
 * block), four 16-column tiles on v_mfma_f32_16x16x4 with each weight converted by the exact v_cvt_f32_f16.  Per (row,
 * output) the sequential-k fp32 chain from the bias, rounded once to fp16, ReLU: every word equals the streamed entry point's on
 * the same nets.  The same arguments, refusals, COEVO_ST_BAD_TASK rule and workspace layout (coevo_dqn16_workspace_bytes). */
int coevo_dqn16_forward_hidden_tiled(const void *slab, const coevo_dqn_task *tasks, int n_tasks, int max_rows_per_task,
                                     int n_rows_total, int C, int n_actions, const uint8_t *frames, int32_t *status,
                                     void *workspace, void *stream);
int coevo_dqn16_forward_argmax_tiled(const void *slab, const coevo_dqn_task *tasks, int n_tasks, int max_rows_per_task,
                                     int n_rows_total, int C, int n_actions, const uint8_t *frames, int32_t *actions,
                                     float *logits, int32_t *status, void *workspace, void *stream);

/* coevo_dqn16_perturb_dist (AtariAgent.clone + Agent.mutate, Atari/atari_agent.py:27-30, agent.py:25-29; np.linalg.norm of
 * diversity_penalty, utils/game_logic_functions.py:12-37) on tiled slabs: parents, children and dist_ref are tiled.  Every
 * entry draws the noise of its canonical index, so the children are coevo_dqn16_relayout of the streamed entry point's children
 * for the same arguments, word for word.  The distance partials keep their shape [n_children][coevo_dqn16_perturb_blocks] and
 * their order - a piece's entries in slab order, then the block of 256 pieces - and equal coevo_dqn16_distance's on the tiled
 * children (not the streamed launch's partials: fp64 sums of the same terms in another grouping). */
int coevo_dqn16_perturb_dist_tiled(const void *parent_slab, const int32_t *parent_idx, void *child_slab, int child_first,
                                   int n_children, int C, int n_actions, const float *sigma_dev, uint64_t seed,
                                   uint32_t stream_lo_first, uint32_t stream_hi, int flags, const int32_t *gen_dev,
                                   int gen_bias, const void *dist_ref, double *dist_partial, void *stream);

#ifdef __cplusplus
}
#endif
#endif
