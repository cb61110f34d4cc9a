// Device pieces of the paddle duel (include/coevo_duel.h states the rules) that more than one translation unit needs: the
// paddle move, the serve, the snapshot word, one world step, the pixel statement and the render loop.  duel_env.hip books one
// agent-step per launch with them; duel_seats.hip books a net's step and a scripted seat's reply in one launch.
#pragma once
#include "coevo_common.hip.h"
#include "philox.hip.h"

#include "../../include/coevo_duel.h"

namespace coevo {

constexpr int DUEL_W = 84, DUEL_PIXELS = DUEL_W * DUEL_W, DUEL_PADDLE_MAX = 72, DUEL_BALL_MAX = 82;
constexpr int DW = COEVO_DUEL_STATE_WORDS;
// VY[off] + 3 for off = 0 .. 12, one nibble each (a table in memory would be a scratch or constant load on the serial path)
constexpr uint64_t DUEL_VY_NIBBLES = 0x6554433322110ull;

__device__ __forceinline__ int duel_move(int p, int a, int n_actions)
{
    int mv = 0;
    if (a >= 0 && a < n_actions) {
        const int m = a % 6;
        mv = m < 2 ? 0 : ((m & 1) ? 4 : -4);
    }
    return min(max(p + mv, 0), DUEL_PADDLE_MAX);
}

__device__ __forceinline__ int duel_vy(int off) { return (int)((DUEL_VY_NIBBLES >> (4 * off)) & 15u) - 3; }

struct DuelBall { int bx, by, vx, vy; };

__device__ inline DuelBall duel_serve(uint64_t seed, int64_t ordinal, int k)
{
    const u32x4 w = philox4x32_10(0xFFFFFFFEu, (uint32_t)k, (uint32_t)ordinal, (uint32_t)((uint64_t)ordinal >> 32) ^ 0x73657276u,
                                  (uint32_t)seed, (uint32_t)(seed >> 32));
    const int i = (int)(w.v[1] & 3u);
    return {41, 8 + (int)(w.v[2] % 68u), (w.v[0] & 1u) ? 3 : -3, i < 2 ? i - 2 : i - 1};
}

__device__ __forceinline__ uint32_t duel_snapshot(int bx, int by, int p0, int p1)
{
    return ((uint32_t)bx & 255u) | ((uint32_t)by & 255u) << 8 | ((uint32_t)p0 & 255u) << 16 | ((uint32_t)p1 & 255u) << 24;
}

// One world step over moved paddles p0, p1 (rules 2 .. 6 of coevo_duel.h): the ball moves, bounces, is returned or scores; a
// point ends the game (ended = t_booked, the agent-steps booked with this one) or is followed by the next serve.  -> r0, the
// reward of first_0 (second_0's is -r0).
__device__ __forceinline__ int duel_world(int &bx, int &by, int &vx, int &vy, int p0, int p1, int &s0, int &s1, int &ended,
                                          int t_booked, uint64_t seed, int64_t ordinal, int points_to_win)
{
    bx += vx;
    by += vy;
    if (by < 0) { by = -by; vy = -vy; }
    if (by > DUEL_BALL_MAX) { by = 2 * DUEL_BALL_MAX - by; vy = -vy; }
    int r0 = 0;
    if (vx < 0 && bx <= 5) {
        const int off = by + 1 - p0;
        if (off >= 0 && off <= 12) { bx = 12 - bx; vx = 3; vy = duel_vy(off); }
        else r0 = -1;
    } else if (vx > 0 && bx >= 77) {
        const int off = by + 1 - p1;
        if (off >= 0 && off <= 12) { bx = 152 - bx; vx = -3; vy = duel_vy(off); }
        else r0 = 1;
    }
    if (r0) {
        if (r0 > 0) ++s0; else ++s1;
        if (max(s0, s1) >= points_to_win) {
            ended = t_booked;
        } else {
            const DuelBall b = duel_serve(seed, ordinal, s0 + s1);
            bx = b.bx; by = b.by; vx = b.vx; vy = b.vy;
        }
    }
    return r0;
}

// the four plane bytes (planes 0 .. 3 = snapshots 0 .. 3) of pixel px as one little-endian word
__device__ __forceinline__ uint32_t duel_pixel(int px, const uint32_t (&snap)[4])
{
    const int y = px / DUEL_W, x = px - y * DUEL_W;
    const bool col0 = (unsigned)(x - 4) < 2u, col1 = (unsigned)(x - 78) < 2u;
    uint32_t word = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int bx = snap[c] & 255, by = (snap[c] >> 8) & 255, p0 = (snap[c] >> 16) & 255, p1 = snap[c] >> 24;
        const bool ball = (unsigned)(x - bx) < 2u && (unsigned)(y - by) < 2u;
        const bool pad = (col0 && (unsigned)(y - p0) < 12u) || (col1 && (unsigned)(y - p1) < 12u);
        word |= (ball ? 255u : (pad ? 160u : 0u)) << (8 * c);
    }
    return word;
}

// every byte of one frame row [84][84][C], once, in 16-byte stores by the workgroup's COEVO_DUEL_THREADS threads: the four
// planes of `snap`, and for C == 6 255 in the plane of the observer (0 first_0, 1 second_0)
__device__ __forceinline__ void duel_render(uint4 *dst, const uint32_t (&snap)[4], int C, int observer)
{
    if (C == 4) {   // one uint4 = 4 pixels
        for (int i = threadIdx.x; i < DUEL_PIXELS / 4; i += COEVO_DUEL_THREADS)
            dst[i] = make_uint4(duel_pixel(4 * i, snap), duel_pixel(4 * i + 1, snap), duel_pixel(4 * i + 2, snap),
                                duel_pixel(4 * i + 3, snap));
    } else {        // C == 6: three uint4 = 8 pixels of 6 bytes: the four planes, then 255 in the observer's plane
        const uint64_t who = observer ? 0xFF00ull : 0x00FFull;
        for (int i = threadIdx.x; i < DUEL_PIXELS / 8; i += COEVO_DUEL_THREADS) {
            uint64_t q[6];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint64_t v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (uint64_t)duel_pixel(8 * i + 4 * h + j, snap) | who << 32;
                q[3 * h] = v[0] | v[1] << 48;
                q[3 * h + 1] = v[1] >> 16 | v[2] << 32;
                q[3 * h + 2] = v[2] >> 32 | v[3] << 16;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
                dst[3 * i + k] = make_uint4((uint32_t)q[2 * k], (uint32_t)(q[2 * k] >> 32), (uint32_t)q[2 * k + 1],
                                            (uint32_t)(q[2 * k + 1] >> 32));
        }
    }
}

// what every duel env-step entry point refuses before it launches (t_min: 1 for the forms that carry an output layer)
inline bool duel_args_ok(const int32_t *state, const double *acc, int n_games, const int64_t *ordinal0, int t, int t_min,
                         const int32_t *limit, const int32_t *row_prev, const int32_t *actions_prev, const int32_t *row_cur,
                         const uint8_t *frames, int C, int n_actions, int points_to_win, int flags)
{
    if (!state || !acc || !ordinal0 || !limit || n_games <= 0 || t < t_min || t > 65535) return false;
    if ((C != 4 && C != 6) || n_actions < 1 || n_actions > COEVO_DQN_LOGIT_STRIDE) return false;
    if (points_to_win < 1 || (flags & ~COEVO_DUEL_CREDIT_OWN)) return false;
    if (t > 0 && (!row_prev || !actions_prev)) return false;
    if (frames && (!row_cur || (reinterpret_cast<uintptr_t>(frames) & 15))) return false;
    return true;
}

}  // namespace coevo
