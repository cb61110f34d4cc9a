"""Statements for the baseline-opponent feature (include/coevo_baseline.h, coevonet_amd/baselines.py): the driver of the C
checker of the PPO policy net (tests/checker16/mlp_checker.c, a real fmaf), the recorded fixture tests/golden/ppo_baseline.npz,
crafted policy nets, and the host game loops - the oracle's own pieces with every seat a callable (obs, k) -> action.  No GPU,
no device library."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from coevonet_amd import baselines as bl
from oracle import ref_port as rp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "checker16", "mlp_checker.c")
FIXTURE = os.path.join(HERE, "golden", "ppo_baseline.npz")
NACT, H = 5, 64
ROLES = ("agent_0", "agent_1", "adversary_0")
ROLE_D = {"agent_0": 10, "agent_1": 10, "adversary_0": 8}
ROLE_SLOT = {"adversary_0": 0, "agent_0": 1, "agent_1": 2}
ST = {"input": 1, "fc1": 2, "fc2": 4, "out": 8}

_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="mlp_checker_"), "libmlp_checker.so")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall", "-o", out,
                               SRC, "-lm"])
        L = C.CDLL(out)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        L.mlp_forward.restype = C.c_int
        L.mlp_forward.argtypes = [fp, C.c_int, fp, fp, ip]
        L.mlp_forward_rows.restype = C.c_int
        L.mlp_forward_rows.argtypes = [fp, C.c_int, fp, C.c_int, C.c_int, ip, fp, ip]
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def mlp_rows(flat, D, obs):
    """obs [n][>= D] -> (actions [n], logits [n][5], status bits [n]) of the checker"""
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    obs = np.ascontiguousarray(obs, dtype=np.float32)
    assert flat.size == bl.mlp_params(D) and obs.ndim == 2 and obs.shape[1] >= D
    n = obs.shape[0]
    actions, logits, st = np.zeros(n, dtype=np.int32), np.zeros((n, NACT), dtype=np.float32), np.zeros(n, dtype=np.int32)
    lib().mlp_forward_rows(_fp(flat), D, _fp(obs), obs.shape[1], n, _ip(actions), _fp(logits), _ip(st))
    return actions, logits, st


def mlp_one(flat, D, obs):
    a, lo, st = mlp_rows(flat, D, np.asarray(obs, dtype=np.float32)[None, :])
    return int(a[0]), lo[0], int(st[0])


@functools.lru_cache(maxsize=None)
def fixture():
    """{role: dict(flat, obs, logits, actions, max_dlogit)} of tests/golden/ppo_baseline.npz (make_golden_ppo.py)"""
    z = np.load(FIXTURE)
    return {r: {k: z[f"{r}.{k}"] for k in ("flat", "obs", "logits", "actions", "max_dlogit")} for r in ROLES}


def fixture_baseline(role):
    return bl.MLPBaseline(fixture()[role]["flat"], ROLE_D[role])


def uniform_obs(n, seed=0):
    """[n][12] float32 uniform(-2, 2) rows, the padding floats poisoned: no kernel may read them"""
    o = np.random.default_rng(seed).uniform(-2, 2, size=(n, 12)).astype(np.float32)
    o[:, 10:] = np.nan
    return o


# ---- crafted policy nets
def parts(D, flat=None):
    """views of a flat policy net: W1 [64][D], b1, W2 [64][64], b2, W3 [5][64], b3"""
    flat = np.zeros(bl.mlp_params(D), dtype=np.float32) if flat is None else flat
    out, off = [], 0
    for shape in ((H, D), (H,), (H, H), (H,), (NACT, H), (NACT,)):
        n = int(np.prod(shape))
        out.append(flat[off:off + n].reshape(shape))
        off += n
    return flat, out


def random_net(D, seed):
    g = np.random.default_rng(seed)
    flat, (W1, b1, W2, b2, W3, b3) = parts(D)
    W1[:], W2[:], W3[:] = g.normal(0, 0.4, W1.shape), g.normal(0, 0.2, W2.shape), g.normal(0, 0.3, W3.shape)
    b1[:], b2[:], b3[:] = g.normal(0, 0.1, H), g.normal(0, 0.1, H), g.normal(0, 0.1, NACT)
    return flat


def crafted(name, D):
    """all_zero: every logit +0 -> action 0; tie: logits (0, 0, 1, 0, 1) -> the first maximum, 2; dead: every hidden unit of
    both layers dead -> the logits are the head's bias; neg_zero: random net with -0.0 weights and biases sprinkled in"""
    flat, (W1, b1, W2, b2, W3, b3) = parts(D)
    if name == "all_zero":
        return flat
    if name == "tie":
        b2[:] = 1.0          # fc1 dead (zero), fc2 = its bias
        W3[2, 7] = W3[4, 7] = 1.0
        return flat
    if name == "dead":
        b1[:], b2[:] = -100.0, -1.0
        W1[:] = 0.0
        W3[:] = np.random.default_rng(3).normal(0, 1, W3.shape)
        b3[:] = (0.25, -1.5, 0.75, 3.0, -0.0)
        return flat
    if name == "neg_zero":
        flat = random_net(D, 17)
        flat[::3] = -0.0
        return flat
    raise KeyError(name)


# ---- the games on the host: the oracle's pieces, every seat a callable (obs, k) -> action
def fc_seat(flat, D):
    flat = np.ascontiguousarray(flat, dtype=np.float32)

    def act(obs, k):
        a, _, st = rp.fc_forward(flat, D, obs[:D])
        assert st == 0 and a >= 0
        return a
    return act


def mlp_seat(flat, D):
    def act(obs, k):
        a, _, st = mlp_one(flat, D, obs[:D])
        assert st == 0
        return a
    return act


def scripted_seat(b, ordinal, slot, n_actions=NACT):
    return lambda obs, k: b.action(ordinal, slot, k, n_actions)


def seat_of(x, role, ordinal):
    """a list entry of BaselineCrossPlay -> its callable in the game with reset ordinal `ordinal`"""
    if isinstance(x, bl.ScriptedBaseline):
        return scripted_seat(x, ordinal, ROLE_SLOT[role])
    if isinstance(x, bl.MLPBaseline):
        return mlp_seat(x.flat, x.D)
    return fc_seat(x, ROLE_D[role])


def play_game_seats(stream, seats, limit=None, max_cycles=25, ordinal=1):
    """rp.play_game_steps with callables in the seats (slot order: adversary_0, agent_0, agent_1) -> (agent_0, agent_1,
    adversary_0) rewards"""
    L = rp.lib()
    s = rp.MpeState()
    L.oracle_mpe_reset(*stream.st, ordinal, C.byref(s))
    cum, acc, act = [0.0] * 3, [0.0] * 3, (C.c_int * 3)(0, 0, 0)
    sel = world_steps = timesteps = 0
    taken = [0, 0, 0]
    obs = np.zeros(10, dtype=np.float32)
    rg, ra = C.c_double(0), C.c_double(0)
    while True:
        agent = sel
        obs[:] = 0
        L.oracle_mpe_observe(C.byref(s), agent, _fp(obs))
        a = int(seats[agent](obs, taken[agent]))
        taken[agent] += 1
        sel = (agent + 1) % 3
        act[agent] = a
        trunc = False
        if sel == 0:
            L.oracle_mpe_world_step(C.byref(s), act, C.byref(rg), C.byref(ra))
            rew = [ra.value, rg.value, rg.value]
            world_steps += 1
            trunc = world_steps >= max_cycles
        else:
            rew = [0.0, 0.0, 0.0]
        cum[agent] = 0.0
        cum = [c + r for c, r in zip(cum, rew)]
        acc[agent] += cum[sel]
        timesteps += 1
        if (limit is not None and timesteps >= limit) or trunc:
            break
    return [acc[1], acc[2], acc[0]]


def crossplay_rewards(lists, E, first, limit, max_cycles=25, seed=rp.ENV_SEED):
    """every game of a BaselineCrossPlay over lists {role: entries} on the host -> rewards [A B C E][3]"""
    A, B, Cn = (len(lists[r]) for r in ROLES)
    out, stream = np.zeros((A * B * Cn * E, 3)), rp.Stream(seed)
    for a in range(A):
        for b in range(B):
            for c in range(Cn):
                for e in range(E):
                    o = first + e
                    seats = [seat_of(lists["adversary_0"][c], "adversary_0", o), seat_of(lists["agent_0"][a], "agent_0", o),
                             seat_of(lists["agent_1"][b], "agent_1", o)]
                    out[((a * B + b) * Cn + c) * E + e] = play_game_seats(stream, seats, limit, max_cycles, o)
    return out


def dqn_seat(flat, C_, n_actions):
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    return lambda frame, k: rp.dqn_forward(flat, C_, n_actions, frame())[0]


def dqn_play_game_seats(seats, C_, n_actions, seed, ordinal, limit):
    """oracle_dqn_play_game's loop on rp.synth_frame / rp.synth_target with callables (frame thunk, k) -> action in the two
    seats -> (first_0, second_0) rewards"""
    cum, rewards, last = [0.0, 0.0], [0.0, 0.0], 0xFF
    for t in range(int(limit)):
        agent, other = t & 1, (t & 1) ^ 1
        action = int(seats[agent](lambda: rp.synth_frame(seed, ordinal, t, last, C_), (t - agent) // 2))
        cum[agent] = 0.0
        hit = 1.0 if action == rp.synth_target(seed, ordinal, t, n_actions) else 0.0
        cum[agent] += hit
        cum[other] += -hit
        last = action
        rewards[agent] += cum[other]
    return rewards


def dqn_crossplay_rewards(first, second, C_, n_actions, E, first_ordinal, limit, seed):
    """every game of a DQNBaselineCrossPlay on the host -> rewards [A B E][3] (third column zero)"""
    def seat(x, parity, o):
        return scripted_seat(x, o, parity, n_actions) if isinstance(x, bl.ScriptedBaseline) else dqn_seat(x, C_, n_actions)
    A, B = len(first), len(second)
    out = np.zeros((A * B * E, 3))
    for a in range(A):
        for b in range(B):
            for e in range(E):
                o = first_ordinal + e
                out[(a * B + b) * E + e, :2] = dqn_play_game_seats([seat(first[a], 0, o), seat(second[b], 1, o)], C_, n_actions,
                                                                   seed, o, limit)
    return out
