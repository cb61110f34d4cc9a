"""Co-ES on the MI355X: drop-in ``evolution_strategy_train(env, args, output_dir)`` (reference
evolutionary_strategy.py:151) over the batched rollout engine.

Reference semantics kept: per generation ``pop`` iterations x 3 roles, each one
perturbed copy of the role's base net (Linear weights/biases only, LayerNorm untouched) playing ONE game against the two
current base nets, in the interleaved order agent_0, agent_1, adversary_0 (game ordinal 3j+role); the role's reward slot
(subject to quirk Q1) is the raw fitness - no rank transform, no antithetic pairs; update theta += lr/(n*sigma) *
sum_i f_i eps_i; optional fitness sharing f/(1+D); 10 evaluation games of the updated trio; adaptive sigma (Q5);
early stopping.  hof_size is unused, as in the reference (Q12).

Two things beyond the reference, both optional and labelled wherever they are reported:
  * the cfg 3 EXTENSION mode of BASELINE.json configs[2] (``args.coevo_antithetic``, ``args.coevo_centered_rank``;
    device_philox only): antithetic pairs (individuals 2m / 2m+1 share one noise stream with opposite signs) and the
    centered-rank transform where the reference has its own normalisation commented out (:133-135).  OFF by default.
  * population sharding over several GPUs: rank r perturbs, plays and partially sums individuals
    [lo, hi); one all-gather of (reward, distance) per individual, one all-gather of the chunk partial sums (the
    update is defined as ES_CHUNKS chunk sums added left to right, so N ranks reproduce one rank bit for bit); the 10
    evaluation games are replicated.

rng modes
  "host_reference"  noise from the global numpy generator in the reference's call order, perturbed nets and the update
                    computed on the host exactly as the reference does (fp64 noise, fp32 GEMV) and uploaded - parity;
  "device_philox"   perturbed nets are materialised once per generation on the device from counter-based noise and the
                    update regenerates the same noise (no noise matrix is ever stored: the reference keeps n x P).
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from . import lib as L
from .es_half import HalfESEngine
from .game_logic import create_agent
from .mpe.simple_adversary import ENV_SEED
from .population import (ES_CHUNKS, N_EVAL, RET_SLOT, ROLE_D, ROLES, SIGMA_ATTR, CoESSchedule, CoESUpdate, NetTable, SlabIO,
                         adapt_mutation_power, co_es_games, half_route, refuse_gauntlet, shard_and_gather,
                         slab_layout)
from .rollout import DeviceRollout, HostEnvRollout, effective_steps


# ---- the reference's per-call helpers under their own names (evolutionary_strategy.py:11-148): sequential, on the host
# except for the games.  The trainer below does the same work batched on the device.
def get_numpy_dtype(precision):
    if precision == "float32":
        return np.float32
    raise ValueError(f"Unsupported precision: {precision}")   # (float16 is out of the parity scope)


def evaluate_current_weights(agent_0, agent_1, adversary, env, args):
    from .genetic_algorithm import evaluate_current_weights as ga_eval
    return ga_eval(agent_0, agent_1, adversary, env, args)


def mutate_weights(env, agent_0, agent_1, adversary, args, role, step, weights_logging_agent_0, weights_logging_agent_1,
                   weights_logging_adversary):
    """one ES individual of `role`: clone the role's base agent, perturb its Linear layers (Agent.mutate_ES), play ONE game
    against the two other base nets -> (the role's slot of play_game's triple, noise, get_weights_ES() of the mutated net)
    (evolutionary_strategy.py:63-116)"""
    from .game_logic import play_game
    base = {"agent_0": agent_0, "agent_1": agent_1, "adversary_0": adversary}
    if role not in base:
        return None
    mutated = base[role].clone(env, args, role=role)
    noise = mutated.mutate_ES(args, role=role, step=step, weights_logging_agent_0=weights_logging_agent_0,
                              weights_logging_agent_1=weights_logging_agent_1,
                              weights_logging_adversary=weights_logging_adversary).astype(get_numpy_dtype(args.precision))
    trio = dict(base)
    trio[role] = mutated
    r = play_game(env=env, player1=trio["agent_0"].model, player2=trio["agent_1"].model,
                  adversary=trio["adversary_0"].model, args=args)
    return r[RET_SLOT[role]], noise, mutated.model.get_weights_ES()


def compute_weight_update(noises, rewards, args, role, individual_weights=None, population_weights=None):
    """(lr / (n sigma_role)) * noises^T fitness, fitness = rewards or rewards / (1 + diversity) -> (update, diversity)
    (evolutionary_strategy.py:120-148: raw rewards, the reference's own normalisation is commented out there)"""
    from .game_logic import diversity_penalty
    dt = get_numpy_dtype(args.precision)
    noises, rewards = np.array(noises, dtype=dt), np.array(rewards, dtype=dt)
    diversity = None
    fitness = rewards
    if args.fitness_sharing:
        diversity = diversity_penalty(individual_weights=individual_weights, population_weights=population_weights, args=args)
        fitness = rewards / (1 + diversity)
    sigma = getattr(args, SIGMA_ATTR[role])
    update = (args.learning_rate / (len(noises) * sigma)) * np.dot(noises.T, fitness)
    return update.astype(dt), diversity


class ESEngine(SlabIO, CoESSchedule, CoESUpdate):
    def __init__(self, pop, limit_train=None, limit_eval=None, max_cycles=25, device="cuda", env_seed=ENV_SEED,
                 rng="device_philox", philox_seed=0, env="device", first_ordinal=1, shard=(0, 1), gather=None,
                 antithetic=False, centered_rank=False, chunks=ES_CHUNKS):
        self.rng_mode, self.philox_seed, self.env_mode, self.device = rng, int(philox_seed), env, device
        self._shard_range(pop, shard, gather, chunks, antithetic, centered_rank, rng)
        self.T_train = effective_steps(limit_train, max_cycles)
        self.T_eval = effective_steps(limit_eval, max_cycles)
        self.n_cycles = (max(self.T_train, self.T_eval) + 2) // 3
        self.first_ordinal = first_ordinal
        self.stride = {r: L.fc_slab_stride(ROLE_D[r]) for r in ROLES}
        self.P = {r: L.fc_param_count(ROLE_D[r]) for r in ROLES}
        self.base, total = slab_layout(ROLES, (("base", 1), ("pert", self.n_local)), self.stride)
        self.slab = torch.zeros(total, dtype=torch.float32, device=device)
        table = NetTable(self.base, self.stride, ROLE_D)
        games, eval_games = co_es_games(table, self.n_local)   # (the evaluation games: a rollout of their own, after the update)
        self.n_main = len(games)
        # env on the host cores: COEVO_HOST_COHORTS alternating cohorts (default 4)
        host_cohorts = None if env == "device" else int(os.environ.get("COEVO_HOST_COHORTS", "4"))
        self._rollout_pair(games, eval_games, table, env_seed, DeviceRollout if env == "device" else HostEnvRollout, host_cohorts)
        f32 = dict(dtype=torch.float32, device=device)
        self.fitness = {r: torch.zeros(pop, **f32) for r in ROLES}
        self.raw = {r: torch.zeros(pop, **f32) for r in ROLES}
        self.dist_local = {r: torch.zeros(max(self.n_local, 1), **f32) for r in ROLES}
        self.div = {r: torch.zeros(1, **f32) for r in ROLES}
        self.sigma = {r: torch.zeros(1, **f32) for r in ROLES}
        self.zero_idx = torch.zeros(max(self.n_local, 1), dtype=torch.int32, device=device)
        self.game_idx = torch.stack([torch.arange(self.n_local, device=device) * 3 + ri for ri in range(3)])
        self.ret_slot = torch.tensor([RET_SLOT[r] for r in ROLES], device=device)
        # per individual (reward in the role's slot, distance to the base net), all roles: what the ranks exchange
        self.stats = torch.zeros(3, pop, 2, dtype=torch.float64, device=device)
        self._partial_layout()
        self.steps_per_generation = 3 * pop * self.T_train + N_EVAL * self.T_eval

    def perturb_device(self, gen, sigmas):
        """this rank's perturbed nets: individual j (global index) of role ri takes noise stream (j, 4*gen + ri)"""
        flags = 1 | (2 if self.antithetic else 0)   # LayerNorm untouched; antithetic pairs in the extension mode
        for ri, r in enumerate(ROLES):
            self.sigma[r].fill_(float(sigmas[r]))
            L.call("coevo_fc_perturb_flags", self._ptr(r, "base"), L._p(self.zero_idx), self._ptr(r, "pert"), 0,
                   self.n_local, ROLE_D[r], L._p(self.sigma[r]), self.philox_seed, self.lo, gen * 4 + ri, flags)

    def _local_distances(self):
        for ri, r in enumerate(ROLES):
            L.call("coevo_fc_distance", self._ptr(r, "base"), self._ptr(r, "pert"), self.n_local, ROLE_D[r],
                   L._p(self.dist_local[r]))
            self.stats[ri, self.lo:self.hi, 1] = self.dist_local[r][:self.n_local]

    def update_device(self, gen, lr, fitness_sharing):
        """the update of generation `gen` from the training rollout's rewards (population.CoESUpdate)"""
        rew = self.ro.rewards if torch.is_tensor(self.ro.rewards) else torch.from_numpy(self.ro.rewards).to(self.device)
        self.co_es_update(rew[self.game_idx, self.ret_slot[:, None]], lr, fitness_sharing)


class ESResult:
    def __init__(self):
        self.rewards = {r: [] for r in ROLES}
        self.diversity, self.sigma_after, self.game_rewards, self.seconds = [], [], [], []
        self.stopped_at = None
        self.fitness = []   # float16 route: per generation the fit16 of the three roles (fp16 values)


def _linear_mask(D):
    """boolean mask over the flat parameter vector: True on Linear weights/biases (the perturbable entries)"""
    from .fcnetwork import param_shapes
    m = []
    for name, shp in param_shapes(D):
        m.append(np.full(int(np.prod(shp)), not name.startswith("ln"), dtype=bool))
    return np.concatenate(m)


class ESTrainer:
    def __init__(self, env, args, rng=None, env_mode=None, collect=True, dist_ctx=None):
        refuse_gauntlet(args, "the Co-ES trainers")
        # float16: rng "device_philox" + the device env on one rank, no extension mode, or a ValueError before anything else
        self.half = half_route(args, "Co-ES with precision", rng, env_mode, dist_ctx, "gather_es",
                               extensions=("coevo_antithetic", "coevo_centered_rank"))
        self.env, self.args, self.collect = env, args, collect
        self.rng = rng or getattr(args, "coevo_rng", "host_reference")
        env_mode = env_mode or getattr(args, "coevo_env", "device")
        self.first_ordinal = getattr(env, "n_resets", 1)
        agents = {r: create_agent(env, args, role=r) for r in ROLES}  # evolutionary_strategy.py:163-165
        shard, gather = shard_and_gather(dist_ctx, "gather_es")
        common = dict(max_cycles=getattr(env, "max_cycles", 25), philox_seed=getattr(args, "coevo_seed", 0),
                      first_ordinal=self.first_ordinal, env_seed=getattr(env, "seed_value", ENV_SEED) or ENV_SEED,
                      chunks=getattr(args, "coevo_es_chunks", ES_CHUNKS))
        if self.half:   # (create_agent built FCNetworkHalf nets; flat() carries fp16 values)
            self.eng = HalfESEngine(args.population, args.max_timesteps_per_episode, args.max_evaluation_steps,
                                    multi_breed=True, **common)
        else:
            self.eng = ESEngine(args.population, args.max_timesteps_per_episode, args.max_evaluation_steps,
                                rng=self.rng, env=env_mode, shard=shard, gather=gather,
                                antithetic=getattr(args, "coevo_antithetic", False),
                                centered_rank=getattr(args, "coevo_centered_rank", False), **common)
        keep = [self.eng.upload(r, "base", 0, agents[r].model.flat()[None]) for r in ROLES]
        torch.cuda.current_stream().synchronize()
        self.base_flat = {r: agents[r].model.flat().copy() for r in ROLES}  # host copy (host_reference mode)
        self.mask = {r: _linear_mask(ROLE_D[r]) for r in ROLES}
        self.res = ESResult()
        self.gen = 0
        self.best = {r: -float("inf") for r in ROLES}
        self.no_improve = {r: 0 for r in ROLES}

    # -- host_reference: the reference's own numpy calls, in its order ------------------------------------------
    def _perturb_host(self):
        args, eng, pop = self.args, self.eng, self.args.population
        self.noises = {r: np.empty((pop, int(self.mask[r].sum())), dtype=np.float32) for r in ROLES}
        pert = {r: np.repeat(self.base_flat[r][None], pop, axis=0) for r in ROLES}
        for j in range(pop):
            for r in ROLES:
                w = self.base_flat[r][self.mask[r]]
                noise = np.random.normal(loc=0.0, scale=getattr(args, SIGMA_ATTR[r]), size=len(w))  # agent.py:52
                pert[r][j, self.mask[r]] = (w + noise).astype(np.float32)   # torch.tensor(..., float32)
                self.noises[r][j] = noise.astype(np.float32)                # evolutionary_strategy.py:74
        keep = [eng.upload(r, "pert", 0, pert[r]) for r in ROLES]
        torch.cuda.current_stream().synchronize()
        self.pert_host = pert

    def _update_host(self):
        args, eng = self.args, self.eng
        rew = eng.rewards_host()
        divs = []
        for ri, r in enumerate(ROLES):
            f = np.array([rew[3 * j + ri, RET_SLOT[r]] for j in range(args.population)], dtype=np.float32)
            div = None
            if args.fitness_sharing:
                base_w = self.base_flat[r][self.mask[r]]
                d = np.array([np.linalg.norm(p[self.mask[r]] - base_w) for p in self.pert_host[r]])
                div = np.sum(np.maximum(0, 1 - d / np.mean(d)))
                f = f / (1 + div)
            sigma = getattr(args, SIGMA_ATTR[r])
            upd = (args.learning_rate / (len(self.noises[r]) * sigma)) * np.dot(self.noises[r].T, f)
            new = self.base_flat[r].copy()
            new[self.mask[r]] = self.base_flat[r][self.mask[r]] + upd.astype(np.float32)
            self.base_flat[r] = new
            divs.append(None if div is None else float(div))
        keep = [eng.upload(r, "base", 0, self.base_flat[r][None]) for r in ROLES]
        torch.cuda.current_stream().synchronize()
        return divs

    def step(self):
        """one generation in the reference's order: perturb (sigma_g) -> 3*pop games -> update -> 10 evaluation games
        -> adaptive sigma / early stopping.  Returns False when early stopping fired."""
        eng, args, res, gen = self.eng, self.args, self.res, self.gen
        t0 = time.perf_counter()
        sigmas = {r: getattr(args, SIGMA_ATTR[r]) for r in ROLES}
        if self.rng == "host_reference":
            self._perturb_host()
        elif self.half:
            eng.perturb(gen, sigmas, args.fitness_sharing)
        else:
            eng.perturb_device(gen, sigmas)
        eng.rollout(gen)
        if self.rng == "host_reference":
            eng.ro.check_status()
            divs = self._update_host()
        else:
            if self.half:
                eng.update(gen, args.learning_rate, args.fitness_sharing)
            else:
                eng.update_device(gen, args.learning_rate, args.fitness_sharing)
            divs = [float(eng.div[r].item()) if args.fitness_sharing else None for r in ROLES] if self.collect else None
        if self.collect:
            res.game_rewards.append(eng.rewards_host()[:eng.n_main].copy())
            res.diversity.append(divs)
            if self.half:
                res.fitness.append([eng.fitness[r].cpu().numpy().copy() for r in ROLES])
        stop = self._finish_generation(gen, eng.evaluate(gen))
        res.seconds.append(time.perf_counter() - t0)
        self.gen += 1
        return not stop

    def _finish_generation(self, gen, ev):
        """bookkeeping after generation `gen`'s evaluation games; returns True when early stopping fires"""
        args, res = self.args, self.res
        for s, r in enumerate(ROLES):
            res.rewards[r].append(ev[s])
        if args.adaptive:
            adapt_mutation_power(args, gen, res.rewards)
        res.sigma_after.append([args.mutation_power_agent_0, args.mutation_power_agent_1, args.mutation_power_adversary])
        if getattr(args, "early_stopping", False):  # evolutionary_strategy.py:320-354
            for s, r in enumerate(ROLES):
                if ev[s] > self.best[r] + args.min_delta:
                    self.best[r], self.no_improve[r] = ev[s], 0
                else:
                    self.no_improve[r] += 1
            for r in ROLES:
                if self.no_improve[r] >= args.patience:
                    res.stopped_at = gen
                    return True
        return False

    def finish(self):
        self.eng.ro.check_status()
        if hasattr(self.env, "n_resets"):
            self.env.n_resets = self.first_ordinal + self.gen * (3 * self.args.population + N_EVAL)
        return self.res

    def base_agents(self):
        """the three trained agents, as the reference returns them (evolutionary_strategy.py:393)"""
        out = []
        state = torch.random.get_rng_state()  # building the agent objects must not advance the reference's RNG stream
        for r in ROLES:
            a = create_agent(self.env, self.args, role=r)
            a.model.set_flat(self.eng.download(r, "base", 0, 1)[0])
            out.append(a)
        torch.random.set_rng_state(state)
        return tuple(out)


def evolution_strategy_train(env, args, output_dir, rng=None, env_mode=None, collect=True, return_result=False,
                             dist_ctx=None):
    """Drop-in for evolutionary_strategy.py:151: returns (agent_0, agent_1, adversary) like the reference; with
    return_result=True also the ESResult history (what the reference only plots).  args.precision "float16" trains half nets
    through HalfESEngine: rng "device_philox" (the argument or args.coevo_rng), device env, one rank, no extension mode;
    anything else raises ValueError before the GPU is touched (DESIGN 6a "Float16 trainers").  With args.game pong_v3 /
    boxing_v2 the DeepQN trainer takes over (dqn_population.dqn_evolution_strategy_train: it returns (base nets, DQNResult));
    there "float16" trains half DeepQN nets through HalfDQNESEngine on one rank, frames synthesised on the device, no
    antithetic pairs, no centered ranks (DESIGN 6a "Float16 DeepQN trainers")."""
    import os
    if getattr(args, "game", "simple_adversary_v3") != "simple_adversary_v3":   # the two-player Atari games
        from .dqn_population import dqn_evolution_strategy_train
        return dqn_evolution_strategy_train(env, args, output_dir, collect=collect, dist_ctx=dist_ctx)
    from .io_utils import ES_FILES, MetricsWriter, save_model, save_state_dicts
    tr = ESTrainer(env, args, rng=rng, env_mode=env_mode, collect=collect, dist_ctx=dist_ctx)
    save = bool(getattr(args, "save", False)) and output_dir is not None
    mw = MetricsWriter(output_dir)
    for _ in range(args.generations):
        go_on = tr.step()
        res, g = tr.res, tr.gen - 1   # one metrics line per generation, written as it finishes
        mw.write(generation=g, eval_rewards={r: res.rewards[r][g] for r in ROLES}, mutation_power=res.sigma_after[g],
                 diversity=res.diversity[g] if g < len(res.diversity) else None,
                 seconds=res.seconds[g] if g < len(res.seconds) else None, stopped=not go_on)
        if not go_on:  # evolutionary_strategy.py:343-354: the reference breaks BEFORE save_model (:357-360), so the
            break      # stopping generation's update is never written
        if save:
            for a, r in zip(tr.base_agents(), ROLES):
                save_model(a, os.path.join(output_dir, ES_FILES[r]))
                save_state_dicts(a, os.path.join(output_dir, ES_FILES[r]), role=r)   # the weights_only-safe twin
    res = tr.finish()
    res.engine = tr.eng
    agents = tr.base_agents()
    return (agents, res) if return_result else agents
