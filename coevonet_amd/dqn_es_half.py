"""Float16 Co-ES generations over DeepQN policies on one GPU: ``HalfDQNESEngine``, the engine of ``args.precision ==
"float16"`` nets for the two-player Atari games (reference Atari/deepqn.py:12-37, 158-172; evolutionary_strategy.py:63-148,
236-272).

The base net and the ``pop`` perturbed nets of the two roles live in ONE fp16 slab (coevo_dqn16_pack's layout).  A generation is:
the perturbed nets (coevo_dqn16_perturb_dist from the role's base net, BatchNorm untouched, noise stream (j, 4 gen + role index),
the distance to the base net fused in when fitness sharing is on), the float16 rollout of the 2 * pop games
(``HalfSynthRollout``: coevo_dqn16_out_synth_step + coevo_dqn16_forward_hidden per agent-step), the update (coevo_es16_fitness,
coevo_dqn_es16_partial - which draws the noise again and rounds it to fp16, where the float32 engine subtracts the base net from
the perturbed nets -, coevo_dqn_es16_apply) and the N_EVAL evaluation games of the updated pair.  The rounding points are the
contract of DESIGN.md 6a "Float16 DeepQN Co-ES".

One rank, one cohort, frames synthesised on the device, ``device_philox`` noise, no antithetic pairs, no centered ranks; the
caller passes sigma per generation, so the host's adaptive rule sits on top: ``DQNESTrainer`` /
``dqn_evolution_strategy_train`` build this engine for ``args.precision == "float16"`` and drive ``generation`` with
``DQNESEngine.generation``'s arguments (dqn_population.dqn_half_route says what they refuse)."""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L
from .atari_synthetic import SYNTH_SEED
from .dqn_ga_half import HalfSynthRollout
from .dqn_population import _DQNSlabIO
from .population import ES_CHUNKS, N_EVAL, ROLES2, NetTable, co_es_games2, mean_eval, slab_layout


class HalfDQNESEngine(_DQNSlabIO):
    """Device-resident float16 base and perturbed nets of first_0 and second_0 and the per-generation steps.

    ``perturb(gen, sigmas, fitness_sharing)`` -> ``rollout(gen)`` -> ``update(gen, lr, fitness_sharing)`` -> ``evaluate(gen)``
    enqueue one generation and synchronise with nothing; ``generation`` does the four, synchronises once and returns the mean
    evaluation pair; ``run`` loops it.  Nets go in and out as flat float32 arrays of fp16 values in parameters() order
    (``DeepQNHalf.flat()``)."""
    _pack_unpack = ("coevo_dqn16_pack", "coevo_dqn16_unpack")   # flat arrays carry fp16 values in float32

    def __init__(self, pop, C, n_actions, T_train, T_eval, device="cuda", env_seed=SYNTH_SEED, philox_seed=0, first_ordinal=1,
                 chunks=ES_CHUNKS, *, shard=(0, 1), gather=None, frames="device", antithetic=False, centered_rank=False,
                 env="synthetic", duel_points=21, duel_credit="next"):
        # what float16 does not cover is refused before the library is loaded
        if tuple(shard) != (0, 1):
            raise ValueError(f"HalfDQNESEngine: precision float16 runs on one rank only, not shard {tuple(shard)}")
        if gather is not None:
            raise ValueError("HalfDQNESEngine: precision float16 runs on one rank only and takes no gather")
        if frames != "device":
            raise ValueError(f'HalfDQNESEngine: precision float16 synthesises frames on the device only, not frames="{frames}"')
        if antithetic:
            raise ValueError("HalfDQNESEngine: antithetic pairs are not built for precision float16")
        if centered_rank:
            raise ValueError("HalfDQNESEngine: the centered-rank transform is not built for precision float16")
        if not (1 <= int(pop) <= 65535 and 1 <= int(chunks) <= 64):
            raise ValueError(f"HalfDQNESEngine: population {pop} (1 .. 65535) or update chunks {chunks} (1 .. 64) out of range")
        from .duel_rollout import duel_env_option   # (imports this module's imports)
        self.duel = duel_env_option("HalfDQNESEngine", env, duel_points, duel_credit, C, frames, shard)
        self.pop, self.chunks = int(pop), int(chunks)
        self.C, self.n_actions, self.device = C, n_actions, device
        self.Cw = C   # (the fp16 slab has one fc1 layout)
        self.T_train, self.T_eval = int(T_train), int(T_eval)
        self.philox_seed = int(philox_seed)
        lib = L.load()
        self.stride = int(lib.coevo_dqn16_slab_stride(C, n_actions))   # 32-bit words
        if self.stride <= 0:
            raise ValueError(f"HalfDQNESEngine: {C} channels / {n_actions} actions is not a DeepQN shape")
        self.P = int(lib.coevo_dqn_param_count(C, n_actions))
        # ---- slab layout: per role [base | pert x pop] -----------------------------------------------------------------
        strides = dict.fromkeys(ROLES2, self.stride)
        self.base, total = slab_layout(ROLES2, (("base", 1), ("pert", self.pop)), strides)
        self.slab = torch.zeros(total, dtype=torch.int32, device=device)
        # ---- the Co-ES game table of the whole population (population.co_es_games2); the evaluation games play the UPDATED
        # base nets, so they are a rollout of their own, on the slab itself (the fp16 slab has no tiled fc1)
        self.per_gen = 2 * self.pop + N_EVAL
        net = NetTable(self.base, strides)
        games, ordinal0, eval_games, eval_ordinal0 = co_es_games2(net, 0, self.pop, first_ordinal, self.pop)
        self.n_main = len(games)
        rollout = HalfSynthRollout
        if self.duel is not None:   # the same tables and forward launches; the env-step launches are the duel's
            import functools
            from .duel_rollout import HalfDuelRollout   # (imports this module)
            rollout = functools.partial(HalfDuelRollout, **self.duel)
        self.ro = rollout(games, net.net_off, ordinal0, C, n_actions, self.slab, env_seed, self.per_gen, device)
        self.ro.set_limits(np.full(self.n_main, self.T_train, dtype=np.int32))
        self.eval_ro = rollout(eval_games, net.net_off, eval_ordinal0, C, n_actions, self.slab, env_seed, self.per_gen, device)
        self.eval_ro.set_limits(np.full(N_EVAL, self.T_eval, dtype=np.int32))
        # ---- small device buffers ----------------------------------------------------------------------------------
        f32 = dict(dtype=torch.float32, device=device)
        self.gen_dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.sigma = torch.zeros(2, **f32)
        self.zero_idx = torch.zeros(self.pop, dtype=torch.int32, device=device)
        self.fitness = [torch.zeros(self.pop, **f32) for _ in ROLES2]   # fit16: fp16 values in fp32 words
        self.dist = [torch.zeros(self.pop, **f32) for _ in ROLES2]      # likewise
        self.div = [torch.zeros(1, **f32) for _ in ROLES2]
        self.game_idx = [(torch.arange(self.pop, dtype=torch.int32, device=device) * 2 + ri).contiguous() for ri in range(2)]
        self.pblocks = int(lib.coevo_dqn16_perturb_blocks(C, n_actions))
        self.dist_partial = [torch.zeros(self.pop * self.pblocks, dtype=torch.float64, device=device) for _ in ROLES2]
        floats = int(lib.coevo_dqn_es16_partial_floats(C, n_actions))
        self.partial = [torch.zeros(self.chunks * floats, **f32) for _ in ROLES2]
        self._dist_gen = None   # the generation whose perturb() left the distances and sharing scores behind
        self.steps_per_generation = 2 * self.pop * self.T_train + N_EVAL * self.T_eval

    # ------------------------------------------------------------------ loading weights (population.SlabIO)
    def _uploaded(self, region):
        self._dist_gen = None   # (the distances perturb() left behind no longer describe the slab)

    # ------------------------------------------------------------------ one generation
    def _finalize_distances(self, ri):
        L.call("coevo_fc16_distance_finalize", L._p(self.dist_partial[ri]), self.pblocks, self.pop, L._p(self.dist[ri]), 0, None)
        L.call("coevo_sharing_score", L._p(self.dist[ri]), self.pop, L._p(self.div[ri]))

    def perturb(self, gen, sigmas, fitness_sharing=False):
        """perturbed net j of role ri = f16(f32(base) + sigma eps) on the conv and Linear entries, noise stream (j, 4 gen + ri):
        DQNESEngine's numbering.  fitness_sharing: the distances to the base net are accumulated while the nets are written
        and turned into the sharing score (update() computes them itself when they are missing)"""
        self.sigma.copy_(torch.tensor([float(sigmas[0]), float(sigmas[1])], dtype=torch.float32))
        for ri, r in enumerate(ROLES2):
            L.call("coevo_dqn16_perturb_dist", self._ptr(r, "base"), L._p(self.zero_idx), self._ptr(r, "pert"), 0, self.pop,
                   self.C, self.n_actions, self.sigma.data_ptr() + 4 * ri, self.philox_seed, 0, gen * 4 + ri, L.DQP_SKIP_BN,
                   None, 0, self._ptr(r, "base") if fitness_sharing else None,
                   L._p(self.dist_partial[ri]) if fitness_sharing else None)
        if fitness_sharing:
            for ri in range(2):
                self._finalize_distances(ri)
        self._dist_gen = gen if fitness_sharing else None

    def rollout(self, gen):
        """the 2 * pop training games of generation `gen` (game ordinal 2j + role in the seeded stream)"""
        self.gen_dev.fill_(gen)
        self.ro.enqueue(self.T_train, self.gen_dev)

    def update(self, gen, lr, fitness_sharing):
        """compute_weight_update (evolutionary_strategy.py:120-148) on half arrays + base += update, on the device; sigma is
        the one perturb() stored"""
        for ri, r in enumerate(ROLES2):
            score = None
            if fitness_sharing:
                if self._dist_gen != gen:   # perturb() ran without the fused distances, or the nets were uploaded
                    L.call("coevo_dqn16_distance", self._ptr(r, "base"), self._ptr(r, "pert"), self.pop, self.C, self.n_actions,
                           L._p(self.dist_partial[ri]))
                    self._finalize_distances(ri)
                score = L._p(self.div[ri])
            L.call("coevo_es16_fitness", L._p(self.ro.acc), L._p(self.game_idx[ri]), ri, self.pop, score, L._p(self.fitness[ri]))
            L.call("coevo_dqn_es16_partial", self.C, self.n_actions, L._p(self.fitness[ri]), self.pop, self.chunks,
                   self.sigma.data_ptr() + 4 * ri, self.philox_seed, 0, gen * 4 + ri, L._p(self.partial[ri]))
            L.call("coevo_dqn_es16_apply", self._ptr(r, "base"), L._p(self.partial[ri]), self.chunks, self.C, self.n_actions,
                   self.pop, self.sigma.data_ptr() + 4 * ri, float(lr))
        self._dist_gen = None   # the base nets moved

    def evaluate(self, gen):
        """the N_EVAL games of the current base pair (evaluate_current_weights), under the ordinals behind the training games"""
        self.gen_dev.fill_(gen)
        self.eval_ro.enqueue(self.T_eval, self.gen_dev)

    def diversity(self):
        """the sharing score of each role in the last generation with fitness sharing (float32)"""
        return [np.float32(self.div[ri].item()) for ri in range(2)]

    def generation(self, gen, sigmas, lr, fitness_sharing=False):
        """one whole generation -> the mean reward pair of its evaluation games"""
        self.perturb(gen, sigmas, fitness_sharing)
        self.rollout(gen)
        self.update(gen, lr, fitness_sharing)
        self.evaluate(gen)
        torch.cuda.synchronize()
        L.raise_on_status(self.ro.status)
        L.raise_on_status(self.eval_ro.status)
        return mean_eval(self.eval_ro.acc.cpu().numpy(), 2)

    def run(self, generations, sigmas, lr, fitness_sharing=False):
        """`generations` whole generations with fixed mutation powers `sigmas` (first_0, second_0) -> {"eval_rewards": [per
        generation mean pair], "diversity": [per generation [float32, float32], or None without fitness sharing]}"""
        out = {"eval_rewards": [], "diversity": []}
        for gen in range(generations):
            out["eval_rewards"].append(self.generation(gen, sigmas, lr, fitness_sharing))
            out["diversity"].append(self.diversity() if fitness_sharing else None)
        return out

    def close(self):
        self.ro.close()
        self.eval_ro.close()
