"""Shared cases and the plain reference for the MPE environment edge tests (tests/test_env_edges_cpu.py, _gpu.py).  No GPU.

The reference is numpy alone: resets are np.random.PCG64(ENV_SEED).advance(...) + simple_adversary.draw_reset (numpy's own
128-bit jump-ahead, not the project's), play is VecSimpleAdversary with the quirk-Q1 credit rule that
test_native_host_env_equals_numpy_env states.  Every comparison built on it is an equality of bit patterns (a NaN matches
any NaN: x86 and gfx950 have different default NaNs)."""
import functools

import numpy as np

from coevonet_amd.mpe import simple_adversary as sa

ENV_SEED = sa.ENV_SEED
STATE_DOUBLES, OBS_STRIDE = 24, 12   # COEVO_MPE_STATE_DOUBLES, COEVO_OBS_STRIDE (asserted against the header by the tests)
HUGE = 0x7fffffff
POISON_ACT = 0x7f7f7f7f

# ------------------------------------------------------------------------------------------------------------- resets
# (ordinal >> 1) * 21 leaves 64 bits from 1756832768924719202 on: ...199, ...200 and ...201 are the last pair and a half below
OVERFLOW_EDGE = 1756832768924719199
RUN7 = tuple(range(4001, 4008))   # 7 consecutive ordinals that start odd: the continuation path of the host reset
ORDINALS = tuple(sorted({0, 1, 2, 3, *RUN7, 2 ** 63 - 1,
                         *[2 ** k + d for k in (16, 31, 32, 33, 40, 53, 62) for d in (-1, 0, 1)],
                         *[OVERFLOW_EDGE + d for d in (0, 1, 2, 4)]}))
DEVICE_ORDINALS = ORDINALS + (2 ** 63 + 2, 2 ** 64 - 1)   # coevo_mpe_reset and coevo_reset_seg take uint64_t
assert ((OVERFLOW_EDGE + 2) >> 1) * 21 < 2 ** 64 <= ((OVERFLOW_EDGE + 4) >> 1) * 21


@functools.lru_cache(maxsize=None)
def ref_reset(ordinal):
    """reset number `ordinal` of the seeded stream -> (goal, apos [3][2], lpos [2][2]): two resets share 21 raw outputs"""
    bg = np.random.PCG64(ENV_SEED)
    bg.advance((int(ordinal) >> 1) * 21)
    rng = np.random.Generator(bg)
    out = sa.draw_reset(rng)
    if ordinal & 1:
        out = sa.draw_reset(rng)
    return out


def lay_out(goal, apos, lpos, vel=None):
    """games -> the [STATE_DOUBLES][n] fp64 state: positions, velocities, landmarks, goal position, zero books (18 .. 21),
    goal index (22) and field 23 zero"""
    goal = np.asarray(goal, dtype=np.int64)
    n = len(goal)
    st = np.zeros((STATE_DOUBLES, n))
    st[0:6] = np.asarray(apos, dtype=np.float64).reshape(n, 6).T
    if vel is not None:
        st[6:12] = np.asarray(vel, dtype=np.float64).reshape(n, 6).T
    st[12:16] = np.asarray(lpos, dtype=np.float64).reshape(n, 4).T
    st[16:18] = np.asarray(lpos, dtype=np.float64)[np.arange(n), goal].T
    st[22] = goal
    return st


def reset_states(ordinals):
    """[STATE_DOUBLES][len(ordinals)]: what a reset of game i at ordinals[i] must leave"""
    r = [ref_reset(int(o)) for o in ordinals]
    return lay_out([x[0] for x in r], np.stack([x[1] for x in r]), np.stack([x[2] for x in r]))


def same_bits(got, want):
    """elementwise: equal bit patterns, or NaN on both sides"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))


def assert_same(got, want, what):
    ok = same_bits(got, want)
    if not ok.all():
        at = tuple(int(i) for i in np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} differ, first at {at}: "
                             f"{np.asarray(got)[at]!r} vs reference {np.asarray(want)[at]!r}")


# ---------------------------------------------------------------------------------------------- crafted state classes
FINITE = ("far_1e4", "on_goal", "mirror", "coincident", "subnormal_obs", "vel_5e-324", "vel_-2.3e-308", "neg_zero", "vel_1e3")
NON_FINITE = ("coord_1e300", "coord_1e39", "coord_nan", "vel_inf")
CLASSES = FINITE[:1] + ("far_1e6",) + FINITE[1:] + NON_FINITE
FUSED_CLASSES = FINITE   # what the whole-game routes play: the x 1e6 field and the non-finite group stay out by name


def craft(name, g):
    """one game of class `name` on top of a reset-like draw from g -> (goal, apos [3][2], vel [3][2], lpos [2][2])"""
    goal, apos, lpos = int(g.integers(2)), g.uniform(-1, 1, (3, 2)), g.uniform(-1, 1, (2, 2))
    vel = np.zeros((3, 2))
    if name == "ordinary":
        pass
    elif name in ("far_1e4", "far_1e6"):
        apos, lpos = apos * float(name[4:]), lpos * float(name[4:])
    elif name == "on_goal":        # agent_0 exactly on the goal: sqrt(0)
        apos[1] = lpos[goal]
    elif name == "mirror":         # agent_1 the mirror image of agent_0 about the goal: the two good distances all but tie
        apos[2] = 2.0 * lpos[goal] - apos[1]
    elif name == "coincident":
        apos[:] = apos[0]
    elif name == "subnormal_obs":  # differences of magnitude 1e-40 (and exact zeros): float32 subnormals
        apos = np.array([[1e-40, -1e-40], [0.0, 0.0], [3e-41, 1e-40]])
        lpos = np.array([[2e-40, -1e-40], [0.0, 1e-40]])
    elif name == "vel_5e-324":
        vel[:] = 5e-324
    elif name == "vel_-2.3e-308":
        vel[:] = -2.3e-308
    elif name == "neg_zero":
        apos, lpos, vel = -np.zeros((3, 2)), -np.zeros((2, 2)), -np.zeros((3, 2))
    elif name == "vel_1e3":
        vel[:] = [[1e3, -1e3], [-1e3, 1e3], [1e3, 1e3]]
    elif name == "coord_1e300":    # dx * dx overflows
        apos[0], apos[2, 1] = [1e300, -1e300], 1e300
    elif name == "coord_1e39":     # a finite fp64 difference past FLT_MAX: the observation is inf
        apos[0], apos[1, 0] = [1e39, -1e39], -1e39
    elif name == "coord_nan":
        apos[1, 0] = np.nan
    elif name == "vel_inf":
        vel[2, 1] = np.inf
    else:
        raise KeyError(name)
    return goal, apos, vel, lpos


class Batch:
    """n games: the classes of `classes` one game each, spread among ordinary reset-like games (n < len(classes): the first n)"""

    def __init__(self, n, seed, classes=CLASSES):
        g = np.random.Generator(np.random.PCG64([int(seed), int(n)]))
        self.n, self.names = n, ["ordinary"] * n
        k = min(n, len(classes))
        for i, name in enumerate(classes[:k]):
            self.names[(i * n) // k + (n // k) // 2] = name
        games = [craft(name, g) for name in self.names]
        self.goal = np.array([x[0] for x in games], dtype=np.int64)
        self.apos, self.vel, self.lpos = (np.stack([x[i] for x in games]) for i in (1, 2, 3))
        self.state = lay_out(self.goal, self.apos, self.lpos, self.vel)
        if "subnormal_obs" in self.names:
            i = self.names.index("subnormal_obs")
            with np.errstate(all="ignore"):
                o = np.abs(np.concatenate([x[i] for x in self.env().observe()]))
            assert ((o > 0) & (o < 2.0 ** -126)).any(), "the subnormal class has no float32 subnormal observation"

    def index(self, name):
        return self.names.index(name)

    def env(self):
        env = sa.VecSimpleAdversary(self.goal, self.apos, self.lpos)
        env.p_vel = self.vel.copy()
        return env


def actions_by_game(n, n_cycles, seed):
    """[n_cycles][n][3] int32 from -1 .. 6 (everything outside 1 .. 4 is a no-op) and one whole game of POISON_ACT words"""
    g = np.random.Generator(np.random.PCG64([int(seed), int(n), 7]))
    a = g.integers(-1, 7, size=(n_cycles, n, 3)).astype(np.int32)
    a[:, n // 3] = POISON_ACT
    return a


def ragged_limits(n, n_cycles, seed):
    """agent-step limits from {0, 1, 2, 3, 4, 3c - 1, 3c, 3c + 1, huge}, c the last cycle but one, in a shuffled order"""
    c = n_cycles - 2
    choices = np.array([0, 1, 2, 3, 4, 3 * c - 1, 3 * c, 3 * c + 1, HUGE], dtype=np.int32)
    g = np.random.Generator(np.random.PCG64([int(seed), int(n), 11]))
    lim = choices[np.arange(n) % len(choices)]
    return lim[g.permutation(n)].copy() if n > 1 else np.array([3 * c + 1], dtype=np.int32)


def shuffled_rows(n, seed):
    """-> (game_rows [n][3], row_game [3n], row_slot [3n]): every (game, slot) at a shuffled row"""
    g = np.random.Generator(np.random.PCG64([int(seed), int(n), 13]))
    game_rows = g.permutation(3 * n).astype(np.int32).reshape(n, 3).copy()
    row_game, row_slot = np.zeros(3 * n, np.int32), np.zeros(3 * n, np.int32)
    for s in range(3):
        row_game[game_rows[:, s]], row_slot[game_rows[:, s]] = np.arange(n), s
    return game_rows, row_game, row_slot


def obs_rows(observed, row_game, row_slot):
    """the [n_rows][OBS_STRIDE] float32 buffer an observe call must leave: columns >= D are +0.0"""
    out = np.zeros((len(row_game), OBS_STRIDE), dtype=np.float32)
    for slot, arr in enumerate(observed):
        m = row_slot == slot
        out[m, :arr.shape[1]] = arr[row_game[m]]
    return out


def ref_play(batch, actions, limits, pos_first):
    """VecSimpleAdversary over `batch` with actions [n_cycles][n][3] and per-game agent-step limits (None: none) -> per cycle
    {"obs": (adv [n][8], a0 [n][10], a1 [n][10]) seen at the start of the cycle, "state": [STATE_DOUBLES][n] after it,
    "rg_prev": [n], "acc": [n][3] by slot}.  Credits (quirk Q1): at agent-step 3c the adversary and at 3c + 1 agent_0 take the
    good reward of the previous world step, at 3c + 2 agent_1 triggers the world step and takes its adversary reward - each
    only while the step index is below the game's limit; a game whose agent_1 no longer acts stands still."""
    n = batch.n
    lim = np.full(n, HUGE, dtype=np.int64) if limits is None else np.asarray(limits, dtype=np.int64)
    keep, sa.INTEGRATE_POS_FIRST = sa.INTEGRATE_POS_FIRST, bool(pos_first)
    try:
        env = batch.env()
        acc, rg_prev, out = np.zeros((n, 3)), np.zeros(n), []
        with np.errstate(all="ignore"):
            for c, acts in enumerate(actions):
                obs = env.observe()
                t0 = 3 * c
                m0, m1, m2 = t0 < lim, t0 + 1 < lim, t0 + 2 < lim
                acc[m0, 0] += rg_prev[m0]
                acc[m1, 1] += rg_prev[m1]
                pos, vel = env.p_pos.copy(), env.p_vel.copy()
                rg, ra = env.step(acts)
                env.p_pos[~m2], env.p_vel[~m2] = pos[~m2], vel[~m2]
                acc[m2, 2] += ra[m2]
                rg_prev[m2] = rg[m2]
                st = lay_out(batch.goal, env.p_pos, batch.lpos, env.p_vel)
                st[18], st[19:22] = rg_prev, acc.T
                out.append({"obs": obs, "state": st, "rg_prev": rg_prev.copy(), "acc": acc.copy()})
        return out
    finally:
        sa.INTEGRATE_POS_FIRST = keep


def triples(acc):
    """[n][3] accumulators by slot -> play_game's order (agent_0, agent_1, adversary_0)"""
    return np.ascontiguousarray(acc[:, [1, 2, 0]])
