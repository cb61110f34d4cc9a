"""Cross-play on the device: every saved agent_0 x agent_1 x adversary, several episodes each, in ONE rollout.

The other half of the reference's main.py is ``--test`` (main.py:193-249): ``load_agent_for_testing``, ten ``play_game`` calls
and a mean.  What the user of a coevolutionary trainer does with it is cross-play - every Hall-of-Fame member of a role against
every member of the others - and ``play_game`` serves that one game at a time: a slab, three packs, a one-game plan and 25
dependent launches per call.  Here the whole table is one game table (population.cross_games), one reset in which every trio
meets the SAME episodes (coevo_mpe_reset_episodes: game g takes ordinal first_ordinal + g % E), one rollout of the existing
kernels and one reduction on the device (coevo_crossplay_reduce: main.py's ``total += reward; total / episodes`` per trio, then
the mean payoff of every net over the trios that seat it).  The host copies the tables back and does nothing else to them.

``CrossPlay``               the three-role simple_adversary games, float32 or float16 nets
``DQNCrossPlay``            the two-player synthetic-Atari games over DeepQN nets
``test_agents``             main.py:193-249 for this package's envs: the mean of `episodes` games of the loaded agents
``cross_play_checkpoints``  whole Hall-of-Fame checkpoints per role -> the ``CrossPlay`` / ``DQNCrossPlay`` result

What cannot be served is refused before the library is loaded.  One rank, env on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L
from .atari_synthetic import SYNTH_SEED, SyntheticAtariAEC
from .mpe.simple_adversary import ENV_SEED, SimpleAdversaryAEC
from .population import ROLE_D, ROLES, ROLES2, NetTable, SlabIO, cross_games, cross_games2, slab_layout
from .rollout import DeviceRollout, RolloutPlan, effective_steps

MAX_GAMES = L.K_XP["COEVO_CROSSPLAY_MAX_GAMES"]   # 2**20: 3 n rows and the two fp64 state buffers (400 MB) stay comfortable


def fc_params(D):
    """coevo_fc_param_count(D) without the library (FCNetwork's parameters() of MPE/fcnetwork.py)"""
    h1, h2, nact = L.K["COEVO_FC_H1"], L.K["COEVO_FC_H2"], L.K["COEVO_FC_NACT"]
    return D * h1 + 3 * h1 + h1 * h2 + 3 * h2 + nact * h2 + nact


def dqn_params(C, n_actions):
    """coevo_dqn_param_count(C, n_actions) without the library (DeepQN's parameters() of Atari/deepqn.py:16-37)"""
    return (C * 32 * 64 + 32) + (32 * 64 * 16 + 64) + (64 * 64 * 9 + 64) + (3136 * 512 + 512) + (512 * n_actions + n_actions) + 320


def _flat(x):
    """an Agent, a net or an array -> its flat float32 parameter vector"""
    x = getattr(x, "model", x)
    return np.ascontiguousarray(x.flat() if hasattr(x, "flat") and callable(x.flat) else x, dtype=np.float32).ravel()


def _role_flats(what, lists, params_of, precision, episodes):
    """the refusals both classes share -> {role: [n][P] float32}"""
    if precision not in ("float32", "float16"):
        raise ValueError(f"Unsupported precision: {precision}")
    if int(episodes) < 1:
        raise ValueError(f"{what}: episodes {episodes} (at least 1)")
    out = {}
    for role, nets in lists.items():
        if nets is None or len(nets) == 0:
            raise ValueError(f"{what}: no net for role {role}")
        flats = [_flat(x) for x in nets]
        for i, f in enumerate(flats):
            if f.size != params_of[role]:
                raise ValueError(f"{what}: net {i} of role {role} has {f.size} parameters, not {params_of[role]}")
        out[role] = flats
    n = int(episodes)
    for f in out.values():
        n *= len(f)
    if n > MAX_GAMES:
        raise ValueError(f"{what}: {n} games (at most {MAX_GAMES})")
    return {role: np.stack(flats) for role, flats in out.items()}


def _check_first_ordinal(what, first_ordinal, episodes_of, bits):
    if int(first_ordinal) < 0:
        raise ValueError(f"{what}: negative first_ordinal {first_ordinal}")
    episodes = episodes_of()
    if int(first_ordinal) + int(episodes) > 1 << bits:
        raise ValueError(f"{what}: first_ordinal {first_ordinal} + {episodes} episodes leaves the {bits}-bit ordinals")


class CrossPlayResult:
    """payoff [A, B, C, 3] (DeepQN: [A, B, 2]) float64 mean rewards per trio in play_game's return order, marginals {role:
    [n_role, slots]} - a net's mean payoff row over the trios that seat it -, rewards [A, B, C, E, 3] ([A, B, E, 2]) per game"""

    def __init__(self, payoff, marginals, rewards):
        self.payoff, self.marginals, self.rewards = payoff, marginals, rewards
        self.n_games = int(np.prod(rewards.shape[:-1]))


class _CrossSlab(SlabIO):
    """one region, "cross", per role: the role's nets in the order they were given"""

    def __init__(self, roles, counts, stride, P, dtype, pack_unpack, net_args, device):
        self.stride, self.P, self.device, self._pack_unpack, self._args = stride, P, device, pack_unpack, net_args
        self.base, total = {}, 0
        for r in roles:   # (slab_layout gives every role the same counts: a call per role, each behind the last)
            b, words = slab_layout((r,), (("cross", counts[r]),), stride)
            self.base[r] = {"cross": total + b[r]["cross"]}
            total += words
        self.slab = torch.zeros(total, dtype=dtype, device=device)

    def _net_args(self, role):
        return self._args(role)


class _CrossBase:
    """what the two classes share: the slab, ``upload``, the reduction and the result"""

    def _build_slab(self, flats, stride, dtype, pack_unpack, net_args):
        self.counts = {r: len(flats[r]) for r in self._roles}
        self.io = _CrossSlab(self._roles, self.counts, stride, self._params, dtype, pack_unpack, net_args, self.device)
        keep = [self.io.upload(r, "cross", 0, flats[r]) for r in self._roles]
        torch.cuda.current_stream().synchronize()
        del keep
        self.table = NetTable(self.io.base, stride, self._D_of)

    def upload(self, role, i, flat):
        """replaces net i of `role`; the next run() plays it"""
        if role not in self._roles:
            raise ValueError(f"{type(self).__name__}: role {role!r} (one of {self._roles})")
        flat = _flat(flat)
        if not 0 <= int(i) < self.counts[role]:
            raise ValueError(f"{type(self).__name__}: net {i} of role {role} (0 .. {self.counts[role] - 1})")
        if flat.size != self._params[role]:
            raise ValueError(f"{type(self).__name__}: {flat.size} parameters, not {self._params[role]}")
        keep = self.io.upload(role, "cross", int(i), flat[None])
        torch.cuda.current_stream().synchronize()
        del keep

    def _reduce_buffers(self, dims):
        f64 = dict(dtype=torch.float64, device=self.device)
        self.dims = dims   # (A, B, C) - C = 1 for the two-player games
        self.payoff = torch.zeros(dims[0] * dims[1] * dims[2], 3, **f64)
        self.marg = [torch.zeros(d, 3, **f64) for d in dims]

    def _reduce(self, rewards, marg_c=True):
        A, B, C = self.dims
        L.call("coevo_crossplay_reduce", L._p(rewards), A, B, C, self.episodes, L._p(self.payoff), L._p(self.marg[0]),
               L._p(self.marg[1]), L._p(self.marg[2]) if marg_c else None)


class CrossPlay(_CrossBase):
    """Every agent_0 x agent_1 x adversary of three lists of nets, ``episodes`` games per trio, in one device rollout.

    A role's list holds flat float32 arrays in parameters() order (``FCNetwork.flat()``; float16: ``FCNetworkHalf.flat()``,
    fp16 values in float32), nets or Agents.  The same weights in two lists are two slab entries.  ``run(first_ordinal)`` plays
    game ((a B + b) C + c) E + e from reset ordinal first_ordinal + e of the seeded stream - what play_game plays when the env
    object stands at that ordinal - for T = effective_steps(limit, max_cycles) agent-steps and returns a ``CrossPlayResult``;
    a net whose forward faults raises play_game's ValueError.  ``upload(role, i, flat)`` replaces a net between runs."""
    _roles, _D_of = ROLES, ROLE_D

    def __init__(self, agent_0, agent_1, adversary, episodes=10, limit=None, max_cycles=25, precision="float32",
                 env_seed=ENV_SEED, device="cuda"):
        self._params = {r: fc_params(ROLE_D[r]) for r in ROLES}
        flats = _role_flats("CrossPlay", {"agent_0": agent_0, "agent_1": agent_1, "adversary_0": adversary}, self._params,
                            precision, episodes)
        self.episodes, self.precision, self.device = int(episodes), precision, device
        self.T = effective_steps(limit, max_cycles)
        half = precision == "float16"
        stride = {r: (L.fc16_slab_stride if half else L.fc_slab_stride)(ROLE_D[r]) for r in ROLES}
        self._build_slab(flats, stride, torch.int32 if half else torch.float32,
                         ("coevo_fc16_pack", "coevo_fc16_unpack") if half else SlabIO._pack_unpack, lambda r: (ROLE_D[r],))
        A, B, C = (self.counts[r] for r in ROLES)
        games, _ = cross_games(self.table, A, B, C, self.episodes)
        self.plan = RolloutPlan(np.array(games), self.table.net_off, self.table.net_D, device=device)
        self.ro = DeviceRollout(self.plan, self.io.slab, env_seed=env_seed, precision=precision)
        self._reduce_buffers((A, B, C))

    def run(self, first_ordinal):
        _check_first_ordinal("CrossPlay", first_ordinal, lambda: self.episodes, 64)
        ro, n = self.ro, self.plan.n_games
        ro.status.zero_()
        ro.set_limits(np.full(n, self.T, dtype=np.int32))
        L.call("coevo_mpe_reset_episodes", L._p(ro.state), n, 0, n, ro.rng, int(first_ordinal), self.episodes)
        ro.run((self.T + 2) // 3)
        ro.check_status()
        self._reduce(ro.rewards)
        A, B, C = self.dims
        marg = {r: self.marg[k].cpu().numpy() for k, r in enumerate(ROLES)}
        return CrossPlayResult(self.payoff.cpu().numpy().reshape(A, B, C, 3), marg,
                               ro.rewards.cpu().numpy().reshape(A, B, C, self.episodes, 3))


class DQNCrossPlay(_CrossBase):
    """``CrossPlay`` for the two-player synthetic-Atari games: every first_0 x second_0 of two lists of DeepQN nets (flat
    arrays in ``DeepQN.flat()`` / ``DeepQNHalf.flat()`` order, nets or Agents), game (a B + b) E + e under reset ordinal
    first_ordinal + e, ``limit`` agent-steps each (required: the synthetic env never terminates).  ``fc1_layout``: the form
    of the slab's fc1 block, "streamed" (play_game's) or "tiled"; the results are the same words."""
    _roles, _D_of = ROLES2, None

    def __init__(self, first, second, C, n_actions, episodes=10, limit=None, precision="float32", env_seed=SYNTH_SEED,
                 fc1_layout="streamed", device="cuda"):
        if limit is None:
            raise ValueError("the synthetic Atari env never terminates: a step limit is required")
        if int(limit) < 0:
            raise ValueError(f"DQNCrossPlay: negative step limit {limit}")
        if fc1_layout not in ("streamed", "tiled"):
            raise ValueError(f'DQNCrossPlay: fc1_layout is "streamed" or "tiled", not {fc1_layout!r}')
        if not (1 <= int(C) <= 6 and 1 <= int(n_actions) <= 32):
            raise ValueError(f"DQNCrossPlay: {C} channels / {n_actions} actions is not a DeepQN shape")
        self.C, self.n_actions = int(C), int(n_actions)
        self._params = dict.fromkeys(ROLES2, dqn_params(self.C, self.n_actions))
        flats = _role_flats("DQNCrossPlay", {"first_0": first, "second_0": second}, self._params, precision, episodes)
        self.episodes, self.precision, self.device, self.T = int(episodes), precision, device, int(limit)
        half, tiled = precision == "float16", fc1_layout == "tiled"
        sym = "coevo_dqn16" if half else "coevo_dqn"
        stride = int(getattr(L.load(), sym + "_slab_stride")(self.C, self.n_actions))
        if stride <= 0:
            raise ValueError(f"DQNCrossPlay: {C} channels / {n_actions} actions is not a DeepQN shape")
        if half:   # the tiled fp16 slab has entry points of its own, the float32 one a bit in the channel argument
            pack, net_args = (sym + "_pack_tiled", sym + "_unpack_tiled") if tiled else (sym + "_pack", sym + "_unpack"), self.C
        else:
            pack, net_args = (sym + "_pack", sym + "_unpack"), self.C | (L.DQN_FC1_TILED if tiled else 0)
        self._build_slab(flats, dict.fromkeys(ROLES2, stride), torch.int32 if half else torch.float32, pack,
                         lambda r: (net_args, self.n_actions))
        A, B = (self.counts[r] for r in ROLES2)
        games, episode = cross_games2(self.table, A, B, self.episodes)
        self._episode = np.asarray(episode, dtype=np.int64)
        if half:
            from .dqn_ga_half import HalfSynthRollout
            self.ro = HalfSynthRollout(games, self.table.net_off, self._episode, self.C, self.n_actions, self.io.slab, env_seed,
                                       0, device, fc1_tiled=tiled)
        else:
            from .dqn_population import SynthRollout
            self.ro = SynthRollout(games, self.table.net_off, self._episode, self.C, self.n_actions, self.io.slab, env_seed, 0,
                                   device, fc1_tiled=tiled)
        self._reduce_buffers((A, B, 1))

    def run(self, first_ordinal):
        _check_first_ordinal("DQNCrossPlay", first_ordinal, lambda: self.episodes, 63)
        ro = self.ro
        ro.status.zero_()
        ro.ordinal0.copy_(torch.from_numpy(int(first_ordinal) + self._episode))
        ro.set_limits(np.full(ro.n_games, self.T, dtype=np.int32))
        ro.enqueue(self.T, None)
        torch.cuda.synchronize()
        L.raise_on_status(ro.status)
        self._reduce(ro.acc, marg_c=False)   # acc is [n][3] with a zero third column: C = 1
        A, B, _ = self.dims
        marg = {r: self.marg[k].cpu().numpy()[:, :2] for k, r in enumerate(ROLES2)}
        return CrossPlayResult(self.payoff.cpu().numpy().reshape(A, B, 3)[..., :2], marg,
                               ro.acc.cpu().numpy().reshape(A, B, self.episodes, 3)[..., :2])


# ---------------------------------------------------------------------------------------------------- main.py --test
def _eval_limit(args):
    return getattr(args, "max_evaluation_steps", None)


def _take_ordinals(env, episodes):
    """the first of the ordinals `episodes` play_game calls on `env` would play, all of them taken: the env object performs the
    resets those calls perform (n_resets moves on by `episodes`, a host env's generator stays in step with it)"""
    first = int(env.n_resets)
    for _ in range(int(episodes)):
        env.reset()
    return first


def _mpe_env_or_raise(env):
    if not (isinstance(env, SimpleAdversaryAEC) and env.seed_value is not None):
        raise ValueError("cross-play runs on this package's seeded simple_adversary env (initialize_env), not on a foreign AEC env")


def _atari_env_or_raise(env):
    from .atari_duel import DuelAEC
    if isinstance(env, DuelAEC):
        raise ValueError("cross-play over the duel env (DuelAEC) is not built into DQNCrossPlay, DQNBaselineCrossPlay and "
                         "test_agents, which play the synthetic Atari env only: use duel_crossplay.DuelCrossPlay, "
                         "duel_test_agents or duel_cross_play_checkpoints")
    if not isinstance(env, SyntheticAtariAEC) or env.seed_value is None:
        raise ValueError("cross-play runs on this package's seeded synthetic Atari env (initialize_env), not on a foreign AEC env")


def _precision_of(nets, half_cls, float_cls):
    """"float16" / "float32" for nets that are all of the half / the float32 class; a mixed set has no device route"""
    if all(isinstance(m, half_cls) for m in nets):
        return "float16"
    if all(isinstance(m, float_cls) and not isinstance(m, half_cls) for m in nets):
        return "float32"
    raise ValueError("cross-play needs nets of one precision: all float32 or all float16")


def test_agents(env, args, episodes=10, opponent=None):
    """main.py:193-249 on this package's envs: ``load_agent_for_testing``, then the mean rewards of `episodes` evaluation games
    (``play_game(..., eval=True)``) - played as ONE rollout, under the reset ordinals the `episodes` play_game calls would have
    taken from `env`, whose ``n_resets`` moves on by `episodes`.  simple_adversary: -> the mean (agent_0, agent_1, adversary)
    triple.  Atari games: ``args.play_against_yourself`` only (the reference's random dummy opponent is not built); the agent
    loaded for agent_0 plays both seats -> the mean (first_0, second_0) pair.  Bit for bit the sums and the division of
    main.py's loop over play_game.

    ``opponent`` (coevonet_amd/baselines.py; None: everything above, to the letter).  Atari games: a scripted baseline that
    plays second_0 against the loaded agent - ``RandomBaseline()`` is main.py's default test path.  simple_adversary: a
    {role: baseline} dict whose baselines replace the loaded agents of those roles."""
    from .game_logic import ATARI_GAMES
    from .io_utils import load_agent_for_testing
    if args.game == "simple_adversary_v3":
        _mpe_env_or_raise(env)
        from .fcnetwork import FCNetwork, FCNetworkHalf
        if opponent is not None:
            from .baselines import BaselineCrossPlay, _is_baseline
            if not isinstance(opponent, dict) or not opponent or set(opponent) - set(ROLES) or \
                    not all(_is_baseline(b) for b in opponent.values()):
                raise ValueError(f"test_agents: for simple_adversary `opponent` is a {{role: baseline}} dict over {ROLES}")
        loaded = load_agent_for_testing(args, env)
        if loaded is None:
            raise ValueError(f"Unsupported algorithm for testing: {args.algorithm}")
        a0, a1, adv = (a.model for a in loaded)
        if opponent is not None:
            seat = {r: [opponent.get(r, m)] for r, m in zip(ROLES, (a0, a1, adv))}
            cp = BaselineCrossPlay(seat["agent_0"], seat["agent_1"], seat["adversary_0"], episodes=episodes,
                                   limit=_eval_limit(args), max_cycles=env.max_cycles, env_seed=env.seed_value)
            res = cp.run(_take_ordinals(env, episodes))
            return tuple(float(v) for v in res.payoff[0, 0, 0])
        precision = _precision_of((a0, a1, adv), FCNetworkHalf, FCNetwork)
        cp = CrossPlay([a0], [a1], [adv], episodes=episodes, limit=_eval_limit(args), max_cycles=env.max_cycles,
                       precision=precision, env_seed=env.seed_value)
        res = cp.run(_take_ordinals(env, episodes))
        return tuple(float(v) for v in res.payoff[0, 0, 0])
    if args.game in ATARI_GAMES:
        _atari_env_or_raise(env)
        if opponent is not None:
            from .baselines import DQNBaselineCrossPlay, ScriptedBaseline
            if not isinstance(opponent, ScriptedBaseline):
                raise ValueError("test_agents: for the Atari games `opponent` is a scripted baseline (RandomBaseline, "
                                 "PeriodicBaseline, ConstantBaseline)")
            loaded = load_agent_for_testing(args, env)
            if loaded is None:
                raise ValueError(f"Unsupported algorithm for testing: {args.algorithm}")
            net = (loaded[0] if isinstance(loaded, (tuple, list)) else loaded).model
            cp = DQNBaselineCrossPlay([net], [opponent], env.C, env.n_actions, episodes=episodes, limit=_eval_limit(args),
                                      env_seed=env.seed_value)
            res = cp.run(_take_ordinals(env, episodes))
            return tuple(float(v) for v in res.payoff[0, 0])
        if not getattr(args, "play_against_yourself", False):
            raise ValueError("test_agents: the Atari games are tested with args.play_against_yourself only (the random dummy "
                             "opponent is not built)")
        from .deepqn import DeepQN, DeepQNHalf
        loaded = load_agent_for_testing(args, env)
        if loaded is None:
            raise ValueError(f"Unsupported algorithm for testing: {args.algorithm}")
        net = (loaded[0] if isinstance(loaded, (tuple, list)) else loaded).model
        precision = _precision_of((net,), DeepQNHalf, DeepQN)
        cp = DQNCrossPlay([net], [net], env.C, env.n_actions, episodes=episodes, limit=_eval_limit(args), precision=precision,
                          env_seed=env.seed_value)
        res = cp.run(_take_ordinals(env, episodes))
        return tuple(float(v) for v in res.payoff[0, 0])
    raise ValueError(f"Unsupported game type: {args.game}")


def cross_play_checkpoints(env, args, paths_by_role, episodes=10, first_ordinal=None):
    """Whole Hall-of-Fame checkpoints against each other: ``paths_by_role`` {role: path} names, per role, a file the trainers
    wrote - a pickled list of Agents (``io_utils.load_agents``) or its ``.state_dict.pth`` twin
    (``io_utils.agents_from_state_dicts``); a single agent counts as a list of one.  EVERY member plays, oldest first, not only
    the newest.  Roles agent_0 / agent_1 / adversary_0 -> ``CrossPlay``, first_0 / second_0 -> ``DQNCrossPlay``; evaluation
    games (``args.max_evaluation_steps``) from ``first_ordinal`` (default: the next resets of `env`, which are then taken)."""
    from .io_utils import STATE_DICT_SUFFIX, agents_from_state_dicts, load_agents
    roles = ROLES if set(paths_by_role) == set(ROLES) else ROLES2 if set(paths_by_role) == set(ROLES2) else None
    if roles is None:
        raise ValueError(f"cross_play_checkpoints: one path for each of {ROLES} or of {ROLES2}, not {sorted(paths_by_role)}")
    (_mpe_env_or_raise if roles is ROLES else _atari_env_or_raise)(env)
    nets = {}
    for r in roles:
        path = paths_by_role[r]
        got = agents_from_state_dicts(env, args, r if roles is ROLES else None, path) if str(path).endswith(STATE_DICT_SUFFIX) \
            else load_agents(path)
        nets[r] = [a.model for a in (got if isinstance(got, (list, tuple)) else [got])]
    if first_ordinal is None:
        first_ordinal = _take_ordinals(env, episodes)
    every = [m for r in roles for m in nets[r]]
    if roles is ROLES:
        from .fcnetwork import FCNetwork, FCNetworkHalf
        cp = CrossPlay(nets["agent_0"], nets["agent_1"], nets["adversary_0"], episodes=episodes, limit=_eval_limit(args),
                       max_cycles=env.max_cycles, precision=_precision_of(every, FCNetworkHalf, FCNetwork),
                       env_seed=env.seed_value)
    else:
        from .deepqn import DeepQN, DeepQNHalf
        cp = DQNCrossPlay(nets["first_0"], nets["second_0"], env.C, env.n_actions, episodes=episodes, limit=_eval_limit(args),
                          precision=_precision_of(every, DeepQNHalf, DeepQN), env_seed=env.seed_value)
    return cp.run(first_ordinal)


test_agents.__test__ = False   # (a library function, not a pytest case, wherever it is imported)
