"""Float16 Co-ES generations on one GPU: ``HalfESEngine``, the engine of ``args.precision == "float16"`` nets for
evolution_strategy_train (reference evolutionary_strategy.py:63-148, 174-177, 236-272; agent.py:31-70;
MPE/fcnetwork.py:202-245).

The base net and the ``pop`` perturbed nets of the three roles live in ONE fp16 slab (coevo_fc16_pack's layout).  A generation
is: the perturbed nets (coevo_fc16_perturb_dist from the role's base net, LayerNorm untouched, noise stream (j, 4 gen + role
index), the distance to the base net fused in when fitness sharing is on), the float16 device rollout of the 3 * pop games
(``DeviceRollout(precision="float16")``), the update (coevo_es16_fitness, coevo_es16_partial - which draws the noise again
and rounds it to fp16, where the float32 engine subtracts the base net from the perturbed nets -, coevo_es16_apply) and the
N_EVAL evaluation games of the updated trio.  The rounding points are the contract of DESIGN.md 6a "Float16 Co-ES".

One rank, device env, ``device_philox`` noise, no antithetic pairs, no centered ranks; the caller passes sigma per generation,
so the host's adaptive rule sits on top.  ``ESTrainer`` / ``evolution_strategy_train`` build this engine under
``args.precision == "float16"`` with ``multi_breed=True``: the three roles' perturbed nets in one launch
(coevo_fc16_perturb_dist_multi) and, with fitness sharing, their distances in one (coevo_fc16_distance_finalize_multi)."""
from __future__ import annotations

import ctypes as ct

import numpy as np
import torch

from . import lib as L
from .mpe.simple_adversary import ENV_SEED
from .population import ES_CHUNKS, N_EVAL, RET_SLOT, ROLE_D, ROLES, CoESSchedule, NetTable, SlabIO, co_es_games, slab_layout
from .rollout import effective_steps


class HalfESEngine(SlabIO, CoESSchedule):
    """Device-resident float16 base and perturbed nets of the three roles and the per-generation steps.

    ``perturb(gen, sigmas)`` -> ``rollout(gen)`` -> ``update(gen, lr, fitness_sharing)`` -> ``evaluate(gen)`` is one
    generation (``generation`` does the four); ``run`` loops them.  Nets go in and out as flat float32 arrays of fp16 values in
    parameters() order (``FCNetworkHalf.flat()``)."""
    _pack_unpack = ("coevo_fc16_pack", "coevo_fc16_unpack")   # flat arrays carry fp16 values in float32

    def __init__(self, pop, limit_train=None, limit_eval=None, max_cycles=25, device="cuda", env_seed=ENV_SEED,
                 philox_seed=0, first_ordinal=1, chunks=ES_CHUNKS, *, rng="device_philox", env="device", shard=(0, 1),
                 antithetic=False, centered_rank=False, multi_breed=False):
        # what float16 does not cover is refused before the library is loaded
        if rng != "device_philox":
            raise ValueError(f'HalfESEngine: precision float16 perturbs with rng="device_philox" only, not "{rng}"')
        if env != "device":
            raise ValueError(f'HalfESEngine: precision float16 has the device env only, not env="{env}"')
        if tuple(shard) != (0, 1):
            raise ValueError(f"HalfESEngine: precision float16 runs on one rank only, not shard {tuple(shard)}")
        if antithetic:
            raise ValueError("HalfESEngine: antithetic pairs are not built for precision float16")
        if centered_rank:
            raise ValueError("HalfESEngine: the centered-rank transform is not built for precision float16")
        if not (1 <= int(pop) <= 65535 and 1 <= int(chunks) <= 64):
            raise ValueError(f"HalfESEngine: population {pop} (1 .. 65535) or update chunks {chunks} (1 .. 64) out of range")
        self.pop, self.chunks = int(pop), int(chunks)
        self.device, self.philox_seed = device, int(philox_seed)
        self.T_train = effective_steps(limit_train, max_cycles)
        self.T_eval = effective_steps(limit_eval, max_cycles)
        self.first_ordinal, self.env_seed = first_ordinal, env_seed
        # ---- slab layout (32-bit words): per role [base | pert x pop] ----------------------------------------------
        self.stride = {r: L.fc16_slab_stride(ROLE_D[r]) for r in ROLES}
        self.P = {r: L.fc_param_count(ROLE_D[r]) for r in ROLES}
        self.base, total = slab_layout(ROLES, (("base", 1), ("pert", self.pop)), self.stride)
        self.slab = torch.zeros(total, dtype=torch.int32, device=device)
        # ---- the Co-ES game table of the whole population on this GPU (population.co_es_games) ----------------------
        self.lo, self.hi, self.n_local, self.env_mode = 0, self.pop, self.pop, "device"
        table = NetTable(self.base, self.stride, ROLE_D)
        games, eval_games = co_es_games(table, self.pop)   # (the evaluation games: a rollout of their own, after the update)
        self.n_main = len(games)
        self._rollout_pair(games, eval_games, table, env_seed, precision="float16")
        # ---- small device buffers ----------------------------------------------------------------------------------
        f32 = dict(dtype=torch.float32, device=device)
        self.fitness = {r: torch.zeros(self.pop, **f32) for r in ROLES}   # fit16: fp16 values in fp32 words
        self.dist = {r: torch.zeros(self.pop, **f32) for r in ROLES}      # likewise
        self.div = {r: torch.zeros(1, **f32) for r in ROLES}
        self.sigma = {r: torch.zeros(1, **f32) for r in ROLES}
        self.zero_idx = torch.zeros(self.pop, dtype=torch.int32, device=device)
        self.game_idx = {r: (torch.arange(self.pop, dtype=torch.int32, device=device) * 3 + ri).contiguous()
                         for ri, r in enumerate(ROLES)}
        self.pblocks = {r: L.fc16_perturb_blocks(ROLE_D[r]) for r in ROLES}
        self.dist_partial = {r: torch.zeros(self.pop * self.pblocks[r], dtype=torch.float64, device=device) for r in ROLES}
        self.partial = {r: torch.zeros(self.chunks * L.es16_partial_floats(ROLE_D[r]), **f32) for r in ROLES}
        self._dist_gen = None   # the generation whose perturb() left the distance partials behind
        self.multi_breed = bool(multi_breed)   # one launch for the three roles' perturbed nets, one for their distances
        self.steps_per_generation = 3 * self.pop * self.T_train + N_EVAL * self.T_eval

    # ------------------------------------------------------------------ loading weights (population.SlabIO)
    def _uploaded(self, region):
        self._dist_gen = None   # (the distance partials perturb() left behind no longer describe the slab)

    # ------------------------------------------------------------------ one generation (rollout, evaluate: population.CoESSchedule)
    def perturb(self, gen, sigmas, fitness_sharing=False):
        """perturbed net j of role ri = f16(f32(base) + sigma eps) on the Linear entries, noise stream (j, 4 gen + ri):
        ESEngine.perturb_device's numbering.  fitness_sharing: the distances to the base net are accumulated while the nets
        are written (update() computes them itself when they are missing)"""
        if self.multi_breed:
            pj = (L.Perturb16Job * 3)()
            for ri, r in enumerate(ROLES):
                self.sigma[r].fill_(float(sigmas[r]))
                pj[ri] = L.Perturb16Job(self._ptr(r, "base"), L._p(self.zero_idx), self._ptr(r, "pert"), L._p(self.sigma[r]),
                                        self._ptr(r, "base") if fitness_sharing else None,
                                        L._p(self.dist_partial[r]) if fitness_sharing else None, 0, self.pop, ROLE_D[r], 0,
                                        gen * 4 + ri, 0)
            L.call("coevo_fc16_perturb_dist_multi", ct.cast(pj, ct.c_void_p), 3, self.philox_seed, 1, None)
            self._dist_gen = gen if fitness_sharing else None
            return
        for ri, r in enumerate(ROLES):
            self.sigma[r].fill_(float(sigmas[r]))
            L.call("coevo_fc16_perturb_dist", self._ptr(r, "base"), L._p(self.zero_idx), self._ptr(r, "pert"), 0, self.pop,
                   ROLE_D[r], L._p(self.sigma[r]), self.philox_seed, 0, gen * 4 + ri, 1, None,
                   self._ptr(r, "base") if fitness_sharing else None,
                   L._p(self.dist_partial[r]) if fitness_sharing else None)
        self._dist_gen = gen if fitness_sharing else None

    def update(self, gen, lr, fitness_sharing):
        """compute_weight_update (evolutionary_strategy.py:120-148) on half arrays + base += update, on the device; sigma is
        the one perturb() stored"""
        self.ro.check_status()
        finalized = fitness_sharing and self.multi_breed and self._dist_gen == gen
        if finalized:   # the fused partials are current: the three roles' distances in one launch
            fj = (L.FinalizeJob * 3)()
            for ri, r in enumerate(ROLES):
                fj[ri] = L.FinalizeJob(L._p(self.dist_partial[r]), L._p(self.dist[r]), None, self.pblocks[r], self.pop, 0, 0)
            L.call("coevo_fc16_distance_finalize_multi", ct.cast(fj, ct.c_void_p), 3)
        for ri, r in enumerate(ROLES):
            D = ROLE_D[r]
            score = None
            if fitness_sharing:
                if self._dist_gen != gen:   # perturb() ran without the fused distances, or the nets were uploaded
                    L.call("coevo_fc16_distance", self._ptr(r, "base"), self._ptr(r, "pert"), self.pop, D,
                           L._p(self.dist_partial[r]))
                if not finalized:
                    L.call("coevo_fc16_distance_finalize", L._p(self.dist_partial[r]), self.pblocks[r], self.pop,
                           L._p(self.dist[r]), 0, None)
                L.call("coevo_sharing_score", L._p(self.dist[r]), self.pop, L._p(self.div[r]))
                score = L._p(self.div[r])
            L.call("coevo_es16_fitness", L._p(self.ro.rewards), L._p(self.game_idx[r]), RET_SLOT[r], self.pop, score,
                   L._p(self.fitness[r]))
            L.call("coevo_es16_partial", D, L._p(self.fitness[r]), self.pop, self.chunks, L._p(self.sigma[r]),
                   self.philox_seed, 0, gen * 4 + ri, L._p(self.partial[r]))
            L.call("coevo_es16_apply", self._ptr(r, "base"), L._p(self.partial[r]), self.chunks, D, self.pop,
                   L._p(self.sigma[r]), float(lr))
        self._dist_gen = None   # the base nets moved

    def diversity(self):
        """the sharing score of each role in the last update() with fitness sharing (float32)"""
        return {r: np.float32(self.div[r].item()) for r in ROLES}

    def generation(self, gen, sigmas, lr, fitness_sharing=False):
        """one whole generation -> the mean reward triple of its evaluation games"""
        self.perturb(gen, sigmas, fitness_sharing)
        self.rollout(gen)
        self.update(gen, lr, fitness_sharing)
        return self.evaluate(gen)

    def run(self, generations, sigmas, lr, fitness_sharing=False):
        """`generations` whole generations with fixed mutation powers `sigmas` {role: sigma} -> {"eval_rewards": [per
        generation mean triple], "diversity": [per generation {role: float32}, or None without fitness sharing]}"""
        out = {"eval_rewards": [], "diversity": []}
        for gen in range(generations):
            out["eval_rewards"].append(self.generation(gen, sigmas, lr, fitness_sharing))
            out["diversity"].append(self.diversity() if fitness_sharing else None)
        return out
