"""Paddle duel: a two-player ball game of the AEC shape of ``pettingzoo.atari`` (agents ``first_0`` / ``second_0`` alternating,
uint8 ``[84, 84, C]`` observations, ``Discrete(n)`` actions) WITH game dynamics, for the DeepQN engines.

It is NOT ALE Pong and does not claim to be: ALE and its ROMs are not part of this build.  It is this project's own statement
of a game, as the MPE env is, in plain integers; the device twin is ``coevo_duel_step`` (csrc/duel_env.hip), whose
contract comment in include/coevo_duel.h states the same rules.  Everything measured on it is labelled duel.

Field: 84 x 84 pixels.  Paddle of first_0: columns 4-5, rows p0 .. p0 + 11; of second_0: columns 78-79, rows p1 .. p1 + 11;
p in [0, 72].  Ball: 2 x 2 at top-left (bx, by), both in [0, 82].  Velocity vx in {-3, +3}, vy in [-3, 3].
first_0 acts at even agent-steps (its action is only stored), second_0 at odd ones, after which the world steps once:
paddles move (MOVE[a mod 6] for 0 <= a < n_actions, clamped), the ball moves, bounces off the top / bottom wall, and at a
paddle plane is either returned (13 offsets -> vy) or scores a point for the other side; a point is followed by serve number
score0 + score1 (Philox-keyed by seed, reset ordinal and serve number) or, at ``points_to_win``, by the end of the game.

Books: PettingZoo's ``_cumulative_rewards`` (the actor's is zeroed when it steps; a world step adds r to both).  Credit rule
"next" (default) is play_atari's quirk, the one the synthetic env keeps: the actor is credited with the cumulative reward of the
agent that acts NEXT, read after its step.  The game is zero-sum, so "next" rewards LOSING a point - the reference's rule, not a
bug of this env.  Credit rule "own" (an extension) credits the actor with its OWN reward of the latest world step - second_0 in
the step that moved the world, first_0 when it steps next - which is the negation of "next" step for step.
"""
from __future__ import annotations

import numpy as np

from .atari_synthetic import ATARI_GAMES, SYNTH_SEED, _Space, philox4x32_10

W = 84
PADDLE_H, PADDLE_MAX, BALL_MAX = 12, 72, 82
X0, X1 = 4, 78                                   # left column of each paddle (two columns wide)
MOVE = (0, 0, -4, 4, -4, 4)
VY = (-3, -2, -2, -1, -1, 0, 0, 0, 1, 1, 2, 2, 3)
SERVE_VY = (-2, -1, 1, 2)
BALL_PIX, PADDLE_PIX = 255, 160
NO_ACTION = 0xFF
CREDITS = ("next", "own")
STATE_WORDS = 16                                 # COEVO_DUEL_STATE_WORDS: the device state of one game (include/coevo_duel.h)


def duel_serve(seed, ordinal, k):
    """serve number k of the game with reset ordinal `ordinal` -> (bx, by, vx, vy)"""
    seed, ordinal = int(seed), int(ordinal)
    w = philox4x32_10(0xFFFFFFFE, int(k), ordinal & 0xFFFFFFFF, ((ordinal >> 32) & 0xFFFFFFFF) ^ 0x73657276,
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return 41, 8 + int(w[2]) % 68, (3 if int(w[0]) & 1 else -3), SERVE_VY[int(w[1]) & 3]


def duel_move(p, a, n_actions):
    a = int(a)
    return min(max(p + (MOVE[a % 6] if 0 <= a < n_actions else 0), 0), PADDLE_MAX)


def snapshot_word(bx, by, p0, p1):
    return (bx & 0xFF) | (by & 0xFF) << 8 | (p0 & 0xFF) << 16 | (p1 & 0xFF) << 24


def render_plane(word):
    """one history snapshot -> the [84, 84] uint8 plane: paddles 160, ball 255 on top, background 0"""
    bx, by, p0, p1 = word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF, (word >> 24) & 0xFF
    f = np.zeros((W, W), dtype=np.uint8)
    f[p0:p0 + PADDLE_H, X0:X0 + 2] = PADDLE_PIX
    f[p1:p1 + PADDLE_H, X1:X1 + 2] = PADDLE_PIX
    f[by:by + 2, bx:bx + 2] = BALL_PIX
    return f


def render_frame(hist, observer, C):
    """four snapshots (oldest first) + the observer (0 first_0, 1 second_0) -> uint8 [84, 84, C]"""
    f = np.zeros((W, W, C), dtype=np.uint8)
    for c in range(4):
        f[:, :, c] = render_plane(int(hist[c]))
    if C == 6:
        f[:, :, 4 + observer] = 255
    return f


class DuelGame:
    """The rules on one game in plain Python ints: the world, the scores and PettingZoo's books.  ``DuelAEC`` wraps one; the
    tests lay its ``words()`` beside the device state."""

    def __init__(self, seed, ordinal, n_actions, points_to_win=21):
        self.seed, self.ordinal, self.n_actions, self.points = int(seed), int(ordinal), int(n_actions), int(points_to_win)
        self.bx, self.by, self.vx, self.vy = duel_serve(seed, ordinal, 0)
        self.p = [36, 36]
        self.score, self.cum = [0, 0], [0, 0]
        self.pending, self.ended = NO_ACTION, 0
        self.hist = [snapshot_word(self.bx, self.by, 36, 36)] * 4
        self.t = 0                                # agent-steps booked

    def world_step(self, a0, a1):
        """-> r = (r0, r1) of this world step"""
        self.p = [duel_move(self.p[0], a0, self.n_actions), duel_move(self.p[1], a1, self.n_actions)]
        self.bx += self.vx
        self.by += self.vy
        if self.by < 0:
            self.by, self.vy = -self.by, -self.vy
        if self.by > BALL_MAX:
            self.by, self.vy = 2 * BALL_MAX - self.by, -self.vy
        r = (0, 0)
        if self.vx < 0 and self.bx <= X0 + 1:
            off = self.by + 1 - self.p[0]
            if 0 <= off <= 12:
                self.bx, self.vx, self.vy = 12 - self.bx, 3, VY[off]
            else:
                r = (-1, 1)
        elif self.vx > 0 and self.bx >= X1 - 1:
            off = self.by + 1 - self.p[1]
            if 0 <= off <= 12:
                self.bx, self.vx, self.vy = 152 - self.bx, -3, VY[off]
            else:
                r = (1, -1)
        if r[0]:
            self.score[0 if r[0] > 0 else 1] += 1
            if max(self.score) >= self.points:
                self.ended = self.t + 1           # the count of agent-steps booked when the game ended (never 0)
            else:
                self.bx, self.by, self.vx, self.vy = duel_serve(self.seed, self.ordinal, self.score[0] + self.score[1])
        self.hist = self.hist[1:] + [snapshot_word(self.bx, self.by, self.p[0], self.p[1])]
        return r

    def step(self, action, own=False):
        """books agent-step self.t (actor = self.t & 1) -> what the actor is credited with; an ended game books nothing"""
        if self.ended:
            return 0
        actor = self.t & 1
        self.cum[actor] = 0
        if actor == 0:
            self.pending = int(action) & 0xFFFFFFFF
            credit = self.cum[1]
        else:
            r = self.world_step(_signed(self.pending), int(action))
            self.pending = NO_ACTION
            self.cum[0] += r[0]
            self.cum[1] += r[1]
            credit = self.cum[0]
        self.t += 1
        return -credit if own else credit

    def words(self):
        """the 16 int32 words of the device state (include/coevo_duel.h)"""
        return np.array([_signed(self.pending), self.bx, self.by, self.vx, self.vy, self.p[0], self.p[1], self.score[0],
                         self.score[1], self.cum[0], self.cum[1], self.ended] + [_signed(h) for h in self.hist], dtype=np.int32)

    def load_words(self, w):
        w = [int(x) for x in w]
        self.pending = w[0] & 0xFFFFFFFF
        self.bx, self.by, self.vx, self.vy = w[1:5]
        self.p, self.score, self.cum, self.ended = w[5:7], w[7:9], w[9:11], w[11]
        self.hist = [x & 0xFFFFFFFF for x in w[12:16]]


def _signed(x):
    x = int(x) & 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


class DuelAEC:
    """AEC env object with the surface of ``SyntheticAtariAEC`` (agents, reset, agent_iter, observe, step, last, the spaces,
    close; ordinal, n_resets, seed_value, C, n_actions) over the duel.  Not a subclass of it: what is gated on the synthetic env
    treats this one as a foreign env."""

    def __init__(self, game="pong_v3", channels=4, points_to_win=21, credit="next", render_mode=None):
        if game not in ATARI_GAMES:
            raise ValueError(f"Unsupported game type: {game}")
        if int(channels) not in (4, 6):
            raise ValueError(f"the duel env renders 4 or 6 channels, not {channels}")
        if int(points_to_win) < 1:
            raise ValueError(f"points_to_win must be at least 1, not {points_to_win}")
        if credit not in CREDITS:
            raise ValueError(f"credit must be one of {CREDITS}, not {credit!r}")
        self.game, self.C, self.n_actions = game, int(channels), ATARI_GAMES[game]
        self.points_to_win, self.credit = int(points_to_win), credit
        self.possible_agents = ["first_0", "second_0"]
        self.agents = list(self.possible_agents)
        self.seed_value = None
        self.n_resets = 0
        self.duel = True

    def observation_space(self, agent):
        return _Space(shape=(W, W, self.C))

    def action_space(self, agent):
        return _Space(n=self.n_actions)

    def reset(self, seed=None, options=None):
        if seed is not None:
            self.seed_value = int(seed)
            self.n_resets = 0
        if self.seed_value is None:
            self.seed_value = SYNTH_SEED
        self.ordinal = self.n_resets
        self.n_resets += 1
        self.state = DuelGame(self.seed_value, self.ordinal, self.n_actions, self.points_to_win)
        self.agent_selection = "first_0"

    @property
    def t(self):
        return self.state.t

    @property
    def _cumulative_rewards(self):
        return {"first_0": float(self.state.cum[0]), "second_0": float(self.state.cum[1])}

    @property
    def terminations(self):
        return {a: bool(self.state.ended) for a in self.agents}

    @property
    def truncations(self):
        return {a: False for a in self.agents}

    def agent_iter(self, max_iter=2 ** 63):
        for _ in range(max_iter):
            yield self.agent_selection

    def observe(self, agent):
        return render_frame(self.state.hist, self.possible_agents.index(agent), self.C)

    def step(self, action):
        if self.state.ended:
            return
        self.state.step(action)
        self.agent_selection = self.possible_agents[self.state.t & 1]

    def last(self):
        """(None, reward, termination, truncation, {}) of the agent that acts next.  "next": its cumulative reward, as
        PettingZoo's last() - what play_atari credits the agent that just acted with.  "own": the reward of the agent that
        just ACTED in the latest world step (zero-sum: minus the other's)."""
        nxt = self.state.t & 1
        reward = float(self.state.cum[nxt]) if self.state.t else 0.0
        if self.credit == "own":
            reward = -reward
        return None, reward, bool(self.state.ended), False, {}

    def snapshot(self):
        """everything the env holds, for laying two env objects side by side"""
        return (self.seed_value, self.ordinal, self.n_resets, self.agent_selection, self.state.t,
                tuple(int(x) for x in self.state.words()))

    def close(self):
        pass


# ------------------------------------------------------------------------------------------------------ scripted players
def duel_tracker_action(obs, player):
    """reads ball and paddle of `player` (0 first_0, 1 second_0) from plane 3 and moves the paddle's centre toward the ball:
    2 (up), 3 (down) or 0 (stay, within 2 pixels)"""
    plane = np.asarray(obs)[:, :, 3]
    ball = np.argwhere(plane == BALL_PIX)
    col = plane[:, (X0, X1)[player]]
    rows = np.flatnonzero(col == PADDLE_PIX)
    if len(ball) == 0 or len(rows) == 0:
        return 0
    ball_c2 = 2 * int(ball[:, 0].min()) + 2          # twice the ball's centre row: rows by, by + 1
    if len(rows) < PADDLE_H:                         # the ball hides part of the paddle: its rows belong to it
        rows = np.union1d(rows, np.flatnonzero(col == BALL_PIX))
    pad_c2 = 2 * int(rows.min()) + PADDLE_H          # twice the paddle's centre
    d = ball_c2 - pad_c2
    return 0 if abs(d) <= 4 else (2 if d < 0 else 3)


class DuelTracker:
    def __init__(self, player):
        self.player = int(player)

    def determine_action(self, obs, args=None):
        return duel_tracker_action(obs, self.player)


class DuelRandom:
    def __init__(self, seed=0, n_actions=6):
        self.rng, self.n_actions = np.random.default_rng(seed), int(n_actions)

    def determine_action(self, obs, args=None):
        return int(self.rng.integers(self.n_actions))
