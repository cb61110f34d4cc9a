"""Drop-in surface of the reference's utils/game_logic_functions.py: ``initialize_env``, ``create_agent``,
``preprocess_observation``, ``play_game``, ``diversity_penalty`` - same names, arguments and errors.

``play_game`` keeps the reference's contract (one env.reset(), one AEC episode, returns the three accumulated rewards
with the reference's attribution).  With this package's own env object the whole episode runs on the GPU in one
batch-of-one rollout; with any other AEC env (e.g. a real PettingZoo one) it walks the AEC loop and only the policy
forward runs on the GPU.
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L
from .agent import MPEAgent
from .atari_synthetic import ATARI_GAMES, SyntheticAtariAEC
from .mpe.simple_adversary import ENV_SEED, SimpleAdversaryAEC
from .rollout import DeviceRollout, RolloutPlan, effective_steps


def initialize_env(args):
    """utils/game_logic_functions.py:41-55 - build the env and do the ONE seeded reset."""
    if args.game == "simple_adversary_v3":
        env = SimpleAdversaryAEC(render_mode="human" if getattr(args, "render", False) else None)
    elif args.game in ATARI_GAMES:
        # ALE / its ROMs are not part of this build (and the reference's Atari loop does not run): the
        # two-player games are served by a SYNTHETIC env of the same AEC shape (coevonet_amd.atari_synthetic).
        # channels: 4 = BASELINE.json's 84x84x4 frames; the reference's wrapper stack (:50-52) would yield 6.
        # args.coevo_atari_env = "duel": the paddle duel (coevonet_amd.atari_duel), a game WITH dynamics - not ALE Pong either
        kind = getattr(args, "coevo_atari_env", "synthetic")
        if kind == "duel":
            from .atari_duel import DuelAEC
            env = DuelAEC(args.game, channels=getattr(args, "coevo_channels", 4),
                          points_to_win=getattr(args, "coevo_duel_points", 21), credit=getattr(args, "coevo_duel_credit", "next"))
        elif kind == "synthetic":
            env = SyntheticAtariAEC(args.game, channels=getattr(args, "coevo_channels", 4))
        else:
            raise ValueError(f'args.coevo_atari_env is "synthetic" or "duel", not {kind!r}')
    else:
        raise ValueError(f"Unsupported game type: {args.game}")
    env.reset(seed=ENV_SEED)
    return env


def create_agent(env, args, role=None):
    if args.game == "simple_adversary_v3":
        return MPEAgent(env, args, role)
    if args.game in ATARI_GAMES:   # utils/game_logic_functions.py:61-62
        from .deepqn import AtariAgent
        return AtariAgent(env, args)
    raise ValueError(f"Unsupported game type: {args.game}")


def preprocess_observation(obs, args):
    """utils/game_logic_functions.py:69-80 for the MPE observation: float16 or float32 as args.precision says"""
    obs = torch.from_numpy(obs)
    if args.precision == "float16":
        return obs.to(torch.float16)
    if args.precision != "float32":
        raise ValueError(f"Unsupported precision: {args.precision}")
    return obs.to(torch.float32)


def diversity_penalty(individual_weights, population_weights, args, sigma=None):
    """fitness-sharing niche count (utils/game_logic_functions.py:12-37) for host-resident weight vectors; the trainers
    use the device kernel coevo_fc_diversity instead."""
    distances = np.array([np.linalg.norm(ind - individual_weights) for ind in population_weights])
    if sigma is None:
        sigma = np.mean(distances)
    return np.sum(np.maximum(0, 1 - distances / sigma))


def _play_mpe_aec(env, player1, player2, adversary, args, eval):
    """play_MPE (:123-212) over a foreign AEC env; forwards on the GPU one step at a time.  Float16 nets are packed once
    per game (HalfPolicySet), so an agent-step moves an observation and an action, not a net."""
    from .fcnetwork import FCNetworkHalf, HalfPolicySet
    rewards = {"agent_0": 0, "agent_1": 0, "adversary_0": 0}
    models = {"agent_0": player1, "agent_1": player2, "adversary_0": adversary}
    half = None
    if all(isinstance(m, FCNetworkHalf) for m in models.values()):
        half = HalfPolicySet(list(models.values()))
        slot_of = {name: i for i, name in enumerate(models)}
    timesteps = 0
    limit = args.max_evaluation_steps if eval else args.max_timesteps_per_episode
    for agent in env.agent_iter():
        if agent not in models:
            raise ValueError(f"Unknown Agent during play_game: {agent}")
        obs = preprocess_observation(env.observe(agent), args)
        if half is not None:
            action = half.forward(slot_of[agent], obs)[1]   # FCNetworkHalf.determine_action, net already on the device
        else:
            action = models[agent].determine_action(obs, args)
        if action > 4:
            raise ValueError(f"ERROR: the action {action} is greater than 4")
        env.step(action)
        _, reward, termination, truncation, _ = env.last()
        rewards[agent] += reward
        timesteps += 1
        if limit is not None and timesteps >= limit:
            break
        if termination or truncation:
            break
    return rewards["agent_0"], rewards["agent_1"], rewards["adversary_0"]


def _play_mpe_device(env, player1, player2, adversary, args, eval):
    """one whole episode on the device; the env object only supplies the game's ordinal in the seeded stream"""
    dev = "cuda"
    ordinal = env.n_resets - 1  # the reset play_game just performed
    s10, s8 = L.fc_slab_stride(10), L.fc_slab_stride(8)
    slab = torch.zeros(2 * s10 + s8, dtype=torch.float32, device=dev)
    for model, off, D in ((player1, 0, 10), (player2, s10, 10), (adversary, 2 * s10, 8)):
        flat = torch.from_numpy(np.ascontiguousarray(model.flat())).to(dev)
        L.call("coevo_fc_pack", L._p(flat), slab.data_ptr() + 4 * off, 1, D)
    plan = RolloutPlan(np.array([[2, 0, 1]]), [0, s10, 2 * s10], [10, 10, 8], device=dev)
    ro = DeviceRollout(plan, slab, env_seed=env.seed_value)
    limit = args.max_evaluation_steps if eval else args.max_timesteps_per_episode
    T = effective_steps(limit, env.max_cycles)
    ro.set_limits([T])
    ro.reset(0, 1, ordinal)
    ro.run((T + 2) // 3)
    ro.check_status()
    r = ro.rewards.cpu().numpy()[0]
    return float(r[0]), float(r[1]), float(r[2])


def _play_mpe_device16(env, player1, player2, adversary, args, eval):
    """_play_mpe_device for three float16 nets: an fp16 slab (coevo_fc16_pack) and a float16 DeviceRollout"""
    dev = "cuda"
    ordinal = env.n_resets - 1  # the reset play_game just performed
    s10, s8 = L.fc16_slab_stride(10), L.fc16_slab_stride(8)
    slab = torch.zeros(2 * s10 + s8, dtype=torch.int32, device=dev)
    for model, off, D in ((player1, 0, 10), (player2, s10, 10), (adversary, 2 * s10, 8)):
        flat = torch.from_numpy(np.ascontiguousarray(model.flat(), dtype=np.float32)).to(dev)
        L.call("coevo_fc16_pack", L._p(flat), slab.data_ptr() + 4 * off, 1, D)
    plan = RolloutPlan(np.array([[2, 0, 1]]), [0, s10, 2 * s10], [10, 10, 8], device=dev)
    ro = DeviceRollout(plan, slab, env_seed=env.seed_value, precision="float16")
    limit = args.max_evaluation_steps if eval else args.max_timesteps_per_episode
    T = effective_steps(limit, env.max_cycles)
    ro.set_limits([T])
    ro.reset(0, 1, ordinal)
    ro.run((T + 2) // 3)
    ro.check_status()
    r = ro.rewards.cpu().numpy()[0]
    return float(r[0]), float(r[1]), float(r[2])


def _play_atari_aec(env, player1, player2, args, eval):
    """play_atari (:84-119) with the signature the call site at :227 uses; forwards on the GPU one step at a time"""
    rewards = {"first_0": 0, "second_0": 0}
    timesteps = 0
    limit = args.max_evaluation_steps if eval else args.max_timesteps_per_episode
    for agent in env.agent_iter():
        obs = env.observe(agent)   # uint8 [84, 84, C]; the HWC -> CHW permute of :78 is folded into the kernel's load
        if agent == "first_0":
            action = player1.determine_action(obs, args)
        elif agent == "second_0":
            action = player2.determine_action(obs, args)
        else:
            raise ValueError(f"Unknown Agent during play_game: {agent}")
        env.step(action)
        _, reward, termination, truncation, _ = env.last()
        rewards[agent] += reward
        timesteps += 1
        if limit is not None and timesteps >= limit:
            break
        if termination or truncation:
            break
    return rewards["first_0"], rewards["second_0"]


def _play_atari_device(env, player1, player2, args, eval, half=False):
    """one whole synthetic-env episode on the device: a two-net slab and a one-game rollout (per agent-step the env-step launch
    with the previous step's output layer in it + conv stack and fc1).  half: two DeepQNHalf players on an fp16 slab
    (coevo_dqn16_pack, HalfSynthRollout)"""
    from .dqn_ga_half import HalfSynthRollout
    from .dqn_population import SynthRollout
    dev = "cuda"
    C, n = env.C, env.n_actions
    sym = "coevo_dqn16" if half else "coevo_dqn"
    stride = int(getattr(L.load(), sym + "_slab_stride")(C, n))
    slab = torch.zeros(2 * stride, dtype=torch.int32 if half else torch.float32, device=dev)
    flat = torch.from_numpy(np.ascontiguousarray(np.stack([player1.flat(), player2.flat()]), dtype=np.float32)).to(dev)
    L.call(sym + "_pack", L._p(flat), L._p(slab), 2, C, n)
    limit = args.max_evaluation_steps if eval else args.max_timesteps_per_episode
    if limit is None:
        raise ValueError("the synthetic Atari env never terminates: a step limit is required")
    ro = (HalfSynthRollout if half else SynthRollout)([(0, 1)], [0, stride], [env.ordinal], C, n, slab, env.seed_value, 0, dev)
    ro.set_limits([int(limit)])
    ro.enqueue(int(limit), None)
    torch.cuda.synchronize()
    L.raise_on_status(ro.status)
    r = ro.acc.cpu().numpy()[0]
    if half:
        _leave_env_stepped(env, int(limit), ro.lanes[0]["actions"].cpu().numpy()[:, 0])
    return float(r[0]), float(r[1])


def _play_duel_device(env, player1, player2, args, eval, half=False):
    """one whole duel episode on the device, as _play_atari_device plays the synthetic env: a two-net slab and a one-game
    DuelRollout / HalfDuelRollout.  The env object is left as the host loop leaves it: state, books, agent_selection."""
    from .duel_rollout import DuelRollout, HalfDuelRollout
    dev = "cuda"
    C, n = env.C, env.n_actions
    limit = args.max_evaluation_steps if eval else args.max_timesteps_per_episode
    if limit is None:
        raise ValueError("the device route of the duel env plays a fixed number of launches: a step limit is required")
    sym = "coevo_dqn16" if half else "coevo_dqn"
    stride = int(getattr(L.load(), sym + "_slab_stride")(C, n))
    slab = torch.zeros(2 * stride, dtype=torch.int32 if half else torch.float32, device=dev)
    flat = torch.from_numpy(np.ascontiguousarray(np.stack([player1.flat(), player2.flat()]), dtype=np.float32)).to(dev)
    L.call(sym + "_pack", L._p(flat), L._p(slab), 2, C, n)
    ro = (HalfDuelRollout if half else DuelRollout)([(0, 1)], [0, stride], [env.ordinal], C, n, slab, env.seed_value, 0, dev,
                                                    points_to_win=env.points_to_win, credit=env.credit)
    ro.set_limits([int(limit)])
    ro.enqueue(int(limit), None)
    torch.cuda.synchronize()
    L.raise_on_status(ro.status)
    r = ro.acc.cpu().numpy()[0]
    words = ro.dstate.cpu().numpy()[0]
    env.state.load_words(words)
    env.state.t = int(words[11]) if words[11] else max(int(limit), 0)   # ended: the agent-steps booked when the game ended
    env.agent_selection = env.possible_agents[env.state.t & 1]
    return float(r[0]), float(r[1])


def _leave_env_stepped(env, T, actions):
    """Two half players walked the AEC loop before their device route existed, and their callers saw the env object stepped:
    leave it where T calls of env.step leave it.  actions[p]: the last action of the player of parity p"""
    from .atari_synthetic import synth_target
    for t in range(max(T - 2, 0), T):   # what the last two steps left in the books holds all of it
        actor, other = env.possible_agents[t & 1], env.possible_agents[1 - (t & 1)]
        hit = 1.0 if int(actions[t & 1]) == synth_target(env.seed_value, env.ordinal, t, env.n_actions) else 0.0
        env._cumulative_rewards[actor] = hit
        env._cumulative_rewards[other] += -hit
        env.last_action, env.t, env.agent_selection = int(actions[t & 1]), t + 1, other


def play_MPE(env, player1, player2, adversary, args, eval):
    """utils/game_logic_functions.py:123-212 - one episode on an ALREADY RESET env (play_game resets): the whole episode
    on the device when env and policies are this package's, else the AEC loop with one device forward per agent-step.
    Three float16 nets take the float16 device rollout (coevo_mpe16_rollout on an fp16 slab)."""
    from .fcnetwork import FCNetwork, FCNetworkHalf
    models = (player1, player2, adversary)
    our_env = isinstance(env, SimpleAdversaryAEC) and env.seed_value is not None
    if our_env and all(isinstance(m, FCNetworkHalf) for m in models):
        return _play_mpe_device16(env, player1, player2, adversary, args, eval)
    if our_env and all(isinstance(m, FCNetwork) and not isinstance(m, FCNetworkHalf) for m in models):
        return _play_mpe_device(env, player1, player2, adversary, args, eval)
    return _play_mpe_aec(env, player1, player2, adversary, args, eval)


def play_atari(env, player1, player2, args, eval=False):
    """utils/game_logic_functions.py:84-119 (its own signature has no eval flag - quirk Q10; the call site at :227 passes
    one, so it is accepted here and selects the step limit as for MPE).  On this package's synthetic env two DeepQN players, or
    two DeepQNHalf players, play the whole episode on the device (float16: an fp16 slab and a HalfSynthRollout); a mixed pair,
    another env or args.coevo_host_aec walk the AEC loop, one forward per agent-step"""
    from .atari_duel import DuelAEC
    from .deepqn import DeepQN, DeepQNHalf
    ours = isinstance(env, SyntheticAtariAEC) or (isinstance(env, DuelAEC) and env.seed_value is not None)
    if ours and not getattr(args, "coevo_host_aec", False):
        device = _play_duel_device if isinstance(env, DuelAEC) else _play_atari_device
        for net in (DeepQN, DeepQNHalf):   # (DeepQNHalf is DeepQN's sibling, not a subclass)
            if isinstance(player1, net) and isinstance(player2, net):
                return device(env, player1, player2, args, eval, half=net is DeepQNHalf)
    return _play_atari_aec(env, player1, player2, args, eval)


def play_game(env, player1, player2, adversary=None, args=None, eval=False):
    """utils/game_logic_functions.py:215-228"""
    env.reset()
    if args.game == "simple_adversary_v3":
        if adversary is None:
            raise ValueError("adversary not specified")
        return play_MPE(env, player1, player2, adversary, args, eval)
    if args.game in ATARI_GAMES:
        return play_atari(env, player1, player2, args, eval)
    raise ValueError(f"Unsupported game type: {args.game}")
