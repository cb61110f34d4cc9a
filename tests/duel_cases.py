"""Statements for the paddle duel (coevonet_amd/atari_duel.py, include/coevo_duel.h): the issue's known answers, a straight-line
restatement of the books, a plain-Python model of one env-step launch over several games (``DuelRef``), crafted states, and host
players for the AEC loop.  No GPU and no library here: tests/test_duel_cpu.py proves these against the rules, tests/test_duel_gpu.py
lays the device beside them."""
import numpy as np

from coevonet_amd import atari_duel as ad

SEED = 1870300
SERVES = [((SEED, 0, 0), (41, 11, 3, 2)), ((SEED, 1, 0), (41, 68, 3, 1)), ((SEED, 1, 3), (41, 37, 3, 2)),
          ((0, 2 ** 63 - 1, 1), (41, 69, 3, 2)), ((2 ** 64 - 1, 5, 40), (41, 51, 3, -1))]
FILL_STATE, FILL_ACC, POISON = 77, 5.5, 0xA5


def books(actions, seed, ordinal, n_actions, points, credit):
    """the returns of play_atari over a list of actions, straight down the rules: PettingZoo's cumulative rewards, then the
    credit rule -> ((first_0, second_0), agent-steps played).  Only the world itself is DuelGame's."""
    g = ad.DuelGame(seed, ordinal, n_actions, points)
    cum, ret, last_r, held = [0, 0], [0, 0], (0, 0), None
    t = 0
    for t, a in enumerate(actions):
        actor = t & 1
        cum[actor] = 0
        if actor == 0:
            held = a
            own = last_r[0]            # first_0 collects what the latest world step gave it
        else:
            g.t = t
            last_r = g.world_step(held, a)
            cum[0] += last_r[0]
            cum[1] += last_r[1]
            own = last_r[1]
        ret[actor] += own if credit == "own" else cum[1 - actor]
        if g.ended:
            break
    return (float(ret[0]), float(ret[1])), (t + 1 if len(actions) else 0)


class DuelRef:
    """one coevo_duel_step launch after another over G games, in plain Python: state words, fp64 returns, frame rows"""

    def __init__(self, ordinal0, limits, gen, per_gen, C, n_actions, seed, points=21, own=False):
        self.G = len(ordinal0)
        self.ordinal = [int(o) + (0 if gen is None else int(gen) * int(per_gen)) for o in ordinal0]
        self.lim = [0 if o < 0 else int(l) for o, l in zip(self.ordinal, limits)]
        self.C, self.n, self.seed, self.points, self.own = C, n_actions, seed, points, own
        self.games = [None] * self.G
        self.state = np.full((self.G, ad.STATE_WORDS), FILL_STATE, dtype=np.int32)
        self.acc = np.full((self.G, 3), FILL_ACC, dtype=np.float64)

    def poke(self, g, **words):
        """overwrite named words of game g (after its reset): bx by vx vy p0 p1 pending score0 score1 cum0 cum1 ended"""
        names = ["pending", "bx", "by", "vx", "vy", "p0", "p1", "score0", "score1", "cum0", "cum1", "ended"]
        for k, v in words.items():
            self.state[g, names.index(k)] = v
        self.games[g].load_words(self.state[g])

    def step(self, t, row_prev, actions, row_cur, frames):
        """frames: [rows][84][84][C] uint8 to render into, or None"""
        rendered = []
        for g in range(self.G):
            if t == 0:
                self.games[g] = ad.DuelGame(self.seed, self.ordinal[g], self.n, self.points)
                self.acc[g] = 0.0
            elif t - 1 < self.lim[g] and not self.games[g].ended:
                game = self.games[g]
                game.t = t - 1
                self.acc[g, (t - 1) & 1] += float(game.step(int(actions[row_prev[g]]), self.own))
            if t == 0 or self.games[g] is not None:
                self.state[g] = self.games[g].words()
            if frames is not None and t < self.lim[g] and not self.games[g].ended:
                frames[row_cur[g]] = ad.render_frame(self.games[g].hist, t & 1, self.C)
                rendered.append(int(row_cur[g]))
        return rendered


def crafted():
    """(name, words to poke, (action of first_0, action of second_0), what must come of the next world step) - the ball one
    step from a wall for every |vy|, at each plane for all 13 offsets and the two nearest misses, wall and plane in one step,
    paddles pushed outward at 0 and 72"""
    out = []
    for v in (1, 2, 3):
        out.append((f"top wall vy -{v}", dict(bx=41, by=v - 1, vx=3, vy=-v), (0, 0), dict(by=1, vy=v)))
        out.append((f"bottom wall vy {v}", dict(bx=41, by=83 - v, vx=-3, vy=v), (0, 0), dict(by=81, vy=-v)))
    for off in range(-1, 14):
        hit = 0 <= off <= 12
        # left plane: the ball arrives at bx = 5 with by = 40; p0 = by + 1 - off
        want = dict(bx=7, vx=3, vy=ad.VY[off]) if hit else dict(score1=1)
        out.append((f"left plane off {off}", dict(bx=8, by=40, vx=-3, vy=0, p0=41 - off, p1=36), (0, 0), want))
        want = dict(bx=75, vx=-3, vy=ad.VY[off]) if hit else dict(score0=1)
        out.append((f"right plane off {off}", dict(bx=74, by=40, vx=3, vy=0, p0=36, p1=41 - off), (1, 1), want))
    # by = 1, vy = -3 -> by = -2 -> 2, vy = 3; the same step reaches the left plane: off = 3 - p0
    out.append(("wall and left plane, hit", dict(bx=8, by=1, vx=-3, vy=-3, p0=0), (0, 0), dict(bx=7, by=2, vx=3, vy=ad.VY[3])))
    out.append(("wall and right plane, miss", dict(bx=76, by=81, vx=3, vy=3, p1=0), (0, 0), dict(score0=1)))
    out.append(("paddles pushed outward", dict(p0=0, p1=72), (2, 3), dict(p0=0, p1=72)))
    out.append(("paddles pushed outward, the other way", dict(p0=72, p1=0), (5, 4), dict(p0=72, p1=0)))
    out.append(("paddles move", dict(p0=2, p1=70), (2, 3), dict(p0=0, p1=72)))
    return out


class ScriptedPlayer:
    """determine_action from a list (the host loop's seat for scripted actions)"""

    def __init__(self, actions):
        self.actions, self.i = list(actions), 0

    def determine_action(self, obs, args=None):
        a = self.actions[self.i]
        self.i += 1
        return a


class OraclePlayer:
    """a DeepQN whose forward is the oracle's (oracle/ref_port.dqn_forward): no action (-1) plays 0, as on the device"""

    def __init__(self, flat, C, n_actions):
        self.net, self.C, self.n = np.ascontiguousarray(flat, dtype=np.float32), C, n_actions

    def determine_action(self, obs, args=None):
        from oracle import ref_port as rp
        a, _ = rp.dqn_forward(self.net, self.C, self.n, obs)
        return max(int(a), 0)


def env_at(ordinal, seed=SEED, game="pong_v3", **kw):
    """a DuelAEC whose NEXT reset plays `ordinal`"""
    env = ad.DuelAEC(game, **kw)
    env.reset(seed=seed)
    env.n_resets = int(ordinal)
    return env
