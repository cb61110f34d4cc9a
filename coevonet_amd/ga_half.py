"""Float16 Co-GA generations on one GPU: ``HalfGAEngine``, the engine of ``args.precision == "float16"`` nets
(reference MPE/fcnetwork.py:13, genetic_algorithm.py:51-345).

The population, the Hall of Fame, the elites and the stale agent of the three roles live in ONE fp16 slab
(coevo_fc16_pack's layout).  A generation is: the float16 device rollout of all 3 * pop * hof games plus the evaluation games
of the previous generation's best trio (``DeviceRollout(precision="float16")``), the selection (coevo_ga_select on
fp16-valued distances), the promotion (coevo_ga16_promote) and the offspring with their stale-agent distances fused in
(coevo_fc16_perturb_dist, coevo_fc16_distance_finalize) - the order and the noise streams of ``GAEngine.breed_device`` on
one GPU.  The rounding points are the float16 contract of DESIGN.md "float16 nets".

One cohort, device env, ``device_philox`` offspring; the caller passes the mutation powers per generation, so the host's
adaptive rule sits on top.  ``GATrainer`` / ``genetic_algorithm_train`` build this engine under ``args.precision == "float16"``
with ``multi_breed=True``: the three roles' children and distances in one launch each (coevo_fc16_perturb_dist_multi,
coevo_fc16_distance_finalize_multi) in place of six.

``hof_mean`` / ``population_sharing``: the two Co-GA extension modes of ``GAEngine`` (not the reference's
algorithm), the pairwise distances in the float16 contract (coevo_fc16_pairwise_distance, include/coevo_sharing16.h)."""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L
from .mpe.simple_adversary import ENV_SEED
from .population import (FUSED_MAX_E, FUSED_MAX_HOF, FUSED_MAX_POP, N_EVAL, ROLE_D, ROLES, CoGASchedule, CoGATail, NetTable,
                         SlabIO, co_ga_games, fused_tail_fits, slab_layout)
from .rollout import DeviceRollout, RolloutPlan, effective_steps


class HalfGAEngine(SlabIO, CoGASchedule, CoGATail):
    """Device-resident float16 population / HoF / elites of the three roles and the per-generation steps.

    ``rollout(gen)`` -> ``select()`` -> ``breed(gen, sigmas)`` is one generation; ``run(generations, sigmas)`` loops them.
    Nets go in and out as flat float32 arrays of fp16 values in parameters() order (``FCNetworkHalf.flat()``)."""
    _pack_unpack = ("coevo_fc16_pack", "coevo_fc16_unpack")   # flat arrays carry fp16 values in float32
    one_reset = True   # the whole population is on this GPU: one reset launch for the three phases
    _promote_entry = "coevo_ga16_promote"
    _perturb_dist_entry = "coevo_fc16_perturb_dist"
    _finalize_entry = "coevo_fc16_distance_finalize"
    _perturb_job = "Perturb16Job"
    _perturb_multi_entry = "coevo_fc16_perturb_dist_multi"
    _finalize_multi_entry = "coevo_fc16_distance_finalize_multi"
    _pairwise_entry = "coevo_fc16_pairwise_distance"
    _pairwise_scratch_entry = "coevo_fc16_pairwise_scratch_doubles"

    def __init__(self, pop, hof, elites, limit_train=None, limit_eval=None, max_cycles=25, device="cuda",
                 env_seed=ENV_SEED, philox_seed=0, first_ordinal=1, *, adaptive=False, shard=(0, 1), env="device",
                 rng="device_philox", multi_breed=False, hof_mean=False, population_sharing=False):
        # the two Co-GA extension modes (NOT the reference's algorithm), as GAEngine has them: fitness over every
        # Hall-of-Fame game, and sharing by a niche count per individual over all pairwise fp16 distances.  Off: nothing changes.
        # (Their limit, COEVO_SHARING_MAX_POP, is the fused tail's FUSED_MAX_POP, refused below.)
        self.hof_mean, self.population_sharing = bool(hof_mean), bool(population_sharing)
        # what float16 does not cover is refused before the library is loaded
        if adaptive:
            raise ValueError("HalfGAEngine: adaptive mutation power is not built for precision float16")
        if tuple(shard) != (0, 1):
            raise ValueError(f"HalfGAEngine: precision float16 runs on one rank only, not shard {tuple(shard)}")
        if env != "device":
            raise ValueError(f'HalfGAEngine: precision float16 has the device env only, not env="{env}"')
        if rng != "device_philox":
            raise ValueError(f'HalfGAEngine: precision float16 breeds with rng="device_philox" only, not "{rng}"')
        if not (pop >= 2 and 1 <= elites <= pop and hof >= 1 and fused_tail_fits(pop, hof, elites)):   # (the fused tail only)
            raise ValueError(f"HalfGAEngine: population {pop} (2 .. {FUSED_MAX_POP}), elites {elites} (1 .. {FUSED_MAX_E}, <= "
                             f"population) or hof {hof} (1 .. {FUSED_MAX_HOF}) out of range")
        self.pop, self.hof, self.E = pop, hof, elites
        self.device, self.philox_seed = device, int(philox_seed)
        self.T_train = effective_steps(limit_train, max_cycles)
        self.T_eval = effective_steps(limit_eval, max_cycles)
        self.n_cycles = (max(self.T_train, self.T_eval) + 2) // 3
        self.first_ordinal, self.env_seed = first_ordinal, env_seed
        # ---- slab layout (32-bit words): per role [pop | hof | elite | stale | hof_tmp] -----------------------
        self.stride = {r: L.fc16_slab_stride(ROLE_D[r]) for r in ROLES}
        self.P = {r: L.fc_param_count(ROLE_D[r]) for r in ROLES}
        self.base, total = slab_layout(ROLES, (("pop", pop), ("hof", hof), ("elite", elites), ("stale", 1), ("hof_tmp", hof)),
                                       self.stride)
        self.slab = torch.zeros(total, dtype=torch.int32, device=device)
        # ---- the Co-GA game table of the whole population on this GPU (population.co_ga_games) ------------------
        self.lo, self.hi, self.n_local, self.env_mode = 0, pop, pop, "device"
        table = NetTable(self.base, self.stride, ROLE_D)
        games, self.n_main = co_ga_games(table, 0, pop, hof)
        self.plan = RolloutPlan(np.array(games), table.net_off, table.net_D, device=device, heavy_rows=16, row_order="class")
        self.ro = DeviceRollout(self.plan, self.slab, env_seed=env_seed, precision="float16")
        # ---- small device buffers ------------------------------------------------------------------------------
        f32 = dict(dtype=torch.float32, device=device)
        self.dist = {r: torch.zeros(pop, **f32) for r in ROLES}          # fp16 values in fp32 words
        self.div = {r: torch.zeros(1, **f32) for r in ROLES}
        self.fitness = {r: torch.zeros(pop, **f32) for r in ROLES}
        self.order = {r: torch.zeros(pop, dtype=torch.int32, device=device) for r in ROLES}
        self.sigma = {r: torch.zeros(1, **f32) for r in ROLES}
        self.best_dist = {r: torch.zeros(1, **f32) for r in ROLES}
        self.pblocks = {r: L.fc16_perturb_blocks(ROLE_D[r]) for r in ROLES}
        self.dist_partial = {r: torch.zeros(pop * self.pblocks[r], dtype=torch.float64, device=device) for r in ROLES}
        self.parent_idx = torch.tensor([c % elites for c in range(pop - 1)], dtype=torch.int32, device=device)
        self._dist_current = False
        if self.population_sharing:
            self._sharing_buffers()
        self.multi_breed = bool(multi_breed)   # breed(): one launch each for the three roles' children and distances
        self.steps_per_generation = 3 * pop * hof * self.T_train + N_EVAL * self.T_eval

    # ------------------------------------------------------------------ loading weights (population.SlabIO)
    def _uploaded(self, region):
        if region in ("pop", "stale"):
            self._dist_current = False   # (the distances breed() left behind no longer describe the slab)

    # ------------------------------------------------------------------ one generation (schedule: population.CoGASchedule)
    def rollout(self, gen):
        """generation `gen`'s games and, riding along from generation 1 on, the evaluation games of generation gen - 1"""
        super().rollout(gen, gen > 0)

    def select(self):
        """fitness sharing + fitness + ranking of the three roles in one launch; the elite ids stay on the device.  Under
        hof_mean / population_sharing: GAEngine's launch-per-step sequence per role (CoGATail._select_shared), the pairwise
        distances in the float16 contract"""
        self.ro.check_status()
        if self.hof_mean or self.population_sharing:
            self._select_shared(L._p(self.ro.rewards), self.pop * self.hof)
        else:
            self._stale_distances(ROLES)
            self._select_roles(lambda ri: L._p(self.ro.rewards), lambda ri: ri * self.pop * self.hof, self.hof)
        self._dist_current = True

    def _stale_distances(self, roles):
        """dist of `roles`: the distances of the population to the stale agent (Q3) in the float16 contract - unless breed()
        left them current (generation 0, or a population loaded from the host: not)"""
        if self._dist_current:
            return
        for r in roles:
            L.call("coevo_fc16_distance", self._ptr(r, "stale"), self._ptr(r, "pop"), self.pop, ROLE_D[r],
                   L._p(self.dist_partial[r]))
            L.call("coevo_fc16_distance_finalize", L._p(self.dist_partial[r]), self.pblocks[r], self.pop,
                   L._p(self.dist[r]), 0, None)

    def breed(self, gen, sigmas):
        """elites -> elite buffer, HoF FIFO, population := [best] + (pop - 1) mutated clones (child c at pop[1 + c] from
        elite[c % E], noise stream (c, 4 gen + role index)), the children's stale-agent distances accumulated while they
        are written; the unchanged best keeps the distance it had"""
        for r in ROLES:
            self.sigma[r].fill_(float(sigmas[r]))
        self._promote_roles(elites_from_pop=True, best_to_pop0=True)
        if self.multi_breed:
            self._breed_children_multi(0, self.pop - 1, [L._p(self.sigma[r]) for r in ROLES], range(gen * 4, gen * 4 + 3))
        else:
            for ri, r in enumerate(ROLES):
                self._breed_role_children(ri, r, 0, self.pop - 1, gen * 4 + ri, None, L._p(self.sigma[r]))
        self._dist_current = True

    def diversity(self):
        """the sharing score of each role in the last select() (float32)"""
        return {r: np.float32(self.div[r].item()) for r in ROLES}

    def run(self, generations, sigmas):
        """`generations` whole generations with fixed mutation powers `sigmas` {role: sigma} -> {"elite_ids": [per generation
        {role: ids}], "eval_rewards": [per generation mean triple], "diversity": [per generation {role: float32}, under
        population_sharing {role: mean_niche()}]}"""
        out = {"elite_ids": [], "eval_rewards": [], "diversity": []}
        for gen in range(generations):
            self.rollout(gen)
            if gen > 0:
                out["eval_rewards"].append(self.eval_rewards())
            self.select()
            out["elite_ids"].append(self.elite_ids())
            out["diversity"].append(dict(zip(ROLES, self.mean_niche())) if self.population_sharing else self.diversity())
            self.breed(gen, sigmas)
        if generations > 0:
            out["eval_rewards"].append(self.eval_only(generations - 1))
        return out
