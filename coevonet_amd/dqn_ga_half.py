"""Float16 Co-GA generations over DeepQN policies on one GPU: ``HalfDQNGAEngine``, the engine of ``args.precision ==
"float16"`` nets for the two-player Atari games (reference Atari/deepqn.py:12-37, genetic_algorithm.py:51-345), and
``HalfSynthRollout``, its rollout over the synthetic env.

The population, the Hall of Fame, the elites and the stale agent of the two roles live in ONE fp16 slab (coevo_dqn16_pack's
layout, ``DQNGAEngine``'s regions per role).  A generation is ``DQNGAEngine``'s own code on one rank with float16 calls: the rollout
of all 2 * pop * hof games plus the evaluation games of the previous generation's best pair (coevo_dqn16_out_synth_step +
coevo_dqn16_forward_hidden per agent-step: three launches, as in float32), then the tail - coevo_ga_select on fp16-valued distances, coevo_ga_adapt_sigma,
the gathers (coevo_net_gather with the stride in words), the offspring with their stale-agent distances fused in
(coevo_dqn16_perturb_dist, coevo_fc16_distance_finalize) and the counter tick - captured once into a hipGraph and replayed.
The rounding points are DESIGN.md 6a "Float16 DeepQN" and "Float16 DeepQN breeding".

One rank, one cohort, frames synthesised on the device.  ``DQNGATrainer`` / ``dqn_genetic_algorithm_train`` build this engine
for ``args.precision == "float16"`` (dqn_population.dqn_half_route says what they refuse)."""
from __future__ import annotations

import os

import torch

from . import lib as L
from .atari_synthetic import SYNTH_SEED
from .dqn_population import DQNGAEngine, SynthRollout


class HalfSynthRollout(SynthRollout):
    """``SynthRollout``'s game and task tables (one cohort) over an fp16 slab: ``net_off`` counts 32-bit words of
    coevo_dqn16_pack's layout.  Three launches per agent-step, the float32 rollout's structure: coevo_dqn16_out_synth_step (the
    output row of the previous step, its booking, the next frames; coevo_synth_step at t = 0) and the conv-stack and fc1 launches
    of coevo_dqn16_forward_hidden.  ``COEVO_DQN16_FUSED_OUT=0``, read at construction, keeps the four-launch route
    (coevo_synth_step + coevo_dqn16_forward_argmax) for A/B runs: the same words in every buffer the engines read.  It
    synchronises with nothing, so a generation can be captured into a graph.  ``fc1_tiled``: the slab's fc1 block is tiled
    (include/coevo_ext.h) and the forward pair is coevo_dqn16_forward_hidden_tiled / coevo_dqn16_forward_argmax_tiled; the
    output row never reads fc1 and keeps its entry point."""

    def __init__(self, game_nets, net_off, ordinal0, C, n_actions, slab, env_seed, ordinals_per_gen, device="cuda", *,
                 fc1_tiled=False):
        super().__init__(game_nets, net_off, ordinal0, C, n_actions, slab, env_seed, ordinals_per_gen, device)
        self.fc1_tiled = bool(fc1_tiled)   # (self.Cw stays the plain channel count: every float16 entry point refuses the bit)
        sfx = "_tiled" if self.fc1_tiled else ""
        self._hidden_entry, self._argmax_entry = "coevo_dqn16_forward_hidden" + sfx, "coevo_dqn16_forward_argmax" + sfx
        ln = self.lanes[0]
        ln["ws"] = torch.zeros(int(L.load().coevo_dqn16_workspace_bytes(ln["n"])) // 4, dtype=torch.float32, device=device)
        self.fused_out = os.environ.get("COEVO_DQN16_FUSED_OUT", "1") != "0"

    def start_timing(self, pairs=512, every=7):
        raise NotImplementedError("HalfSynthRollout: the float16 forward has no timed form")

    def _enqueue_lane(self, ln, T, g, stream, timed):
        for t in range(T + 1):
            self.enqueue_step(ln, t, T, g, stream)

    def enqueue_step(self, ln, t, T, g, stream):
        """the launches of agent-step t of a T-step rollout (t = T: the closing bookkeeping call alone)"""
        m, lib = ln["n"], L.load()
        p, q = t & 1, (t - 1) & 1
        env = (L._p(self.gstate), L._p(self.acc), m, L._p(self.ordinal0), g, self.ordinals_per_gen, t, L._p(self.limit),
               L._p(ln["rows"][q]) if t else None, ln["actions"][q].data_ptr() if t else None,
               L._p(ln["rows"][p]) if t < T else None, L._p(ln["frames"]) if t < T else None, self.C, self.n_actions,
               self.env_seed)
        fwd = (L._p(self.slab), L._p(ln["tasks"][p]), ln["n_tasks"][p], ln["max_rows"][p], m, self.C, self.n_actions,
               L._p(ln["frames"]))
        if t and self.fused_out:   # the output layer of step t-1 rides in the env-step launch
            L._check(lib.coevo_dqn16_out_synth_step(*env, L._p(self.slab), L._p(ln["tasks"][q]), ln["n_tasks"][q], m,
                                                    L._p(ln["ws"]), L._p(self.status), stream), "coevo_dqn16_out_synth_step")
        else:
            L._check(lib.coevo_synth_step(*env, stream), "coevo_synth_step")
        if t < T and self.fused_out:
            L._check(getattr(lib, self._hidden_entry)(*fwd, L._p(self.status), L._p(ln["ws"]), stream), self._hidden_entry)
        elif t < T:
            L._check(getattr(lib, self._argmax_entry)(*fwd, ln["actions"][p].data_ptr(), None, L._p(self.status),
                                                      L._p(ln["ws"]), stream), self._argmax_entry)

    def weight_bytes_per_round(self):
        """algorithmic bytes of one round (two agent-steps): every distinct acting fp16 weight set once per agent-step + the
        frames"""
        net_bytes = int(L.load().coevo_dqn16_slab_stride(self.C, self.n_actions)) * 4
        nets = sum(len({int(t["net_off"]) for t in tn}) for tn in self.tasks_np)
        return nets * net_bytes + 2 * self.n_games * 84 * 84 * self.C


class HalfDQNGAEngine(DQNGAEngine):
    """``DQNGAEngine`` on one rank over an fp16 slab (coevo_dqn16_pack's layout): its constructor, game table, ``load_initial``,
    tail, ``step`` and ``eval_only``, with the float16 entry points and three hooks - the rollout, the distances of the initial
    population and the children of a role.  Nets go in and out as flat float32 arrays of fp16 values in parameters() order
    (``DeepQNHalf.flat()``).

    ``fc1_layout``: "streamed" (the default) or "tiled" - the slab's fc1 block in the form of include/coevo_ext.h, for
    v_mfma_f32_16x16x4 tiles in the rollout's fc1 launch.  Upload / download, the rollout's forward pair and the children then go
    through the ``*_tiled`` entry points; the distances of the initial population stay coevo_dqn16_distance (both nets have one
    form).  Every result - rewards, fitness, distances, downloaded nets - is the streamed engine's, bit for bit.  ``fc1_tiled``
    says which form the slab has."""
    _pack_unpack = ("coevo_dqn16_pack", "coevo_dqn16_unpack")   # flat arrays carry fp16 values in float32
    _slab_dtype = torch.int32
    _stride_entry, _pblocks_entry = "coevo_dqn16_slab_stride", "coevo_dqn16_perturb_blocks"
    _finalize_entry = "coevo_fc16_distance_finalize"
    _fc1_tileable = False
    _saves_sigma_prev = False   # one rank: no elite is ever rebuilt

    def __init__(self, pop, hof, elites, C, n_actions, T_train, T_eval, device="cuda", env_seed=SYNTH_SEED, philox_seed=0,
                 first_ordinal=1, capacity=1024, sigmas=(0.05, 0.05), sig_min=0.001, sig_max=0.2, adaptive=True, *,
                 shard=(0, 1), gather=None, frames="device", fc1_layout="streamed", env="synthetic", duel_points=21,
                 duel_credit="next"):
        # what float16 does not cover is refused before the library is loaded
        if tuple(shard) != (0, 1):
            raise ValueError(f"HalfDQNGAEngine: precision float16 runs on one rank only, not shard {tuple(shard)}")
        if frames != "device":
            raise ValueError(f'HalfDQNGAEngine: precision float16 synthesises frames on the device only, not frames="{frames}"')
        if gather is not None:
            raise ValueError("HalfDQNGAEngine: precision float16 runs on one rank only and takes no gather")
        if not (1 <= elites <= pop and hof >= 1):
            raise ValueError(f"HalfDQNGAEngine: elites {elites} (1 .. population {pop}) or hof {hof} (>= 1) out of range")
        if fc1_layout not in ("streamed", "tiled"):
            raise ValueError(f'HalfDQNGAEngine: fc1_layout is "streamed" or "tiled", not {fc1_layout!r}')
        self._half_tiled = fc1_layout == "tiled"   # (the constructor below builds the rollout: set first)
        if self._half_tiled:
            self._pack_unpack = ("coevo_dqn16_pack_tiled", "coevo_dqn16_unpack_tiled")
        super().__init__(pop, hof, elites, C, n_actions, T_train, T_eval, device=device, env_seed=env_seed,
                         philox_seed=philox_seed, first_ordinal=first_ordinal, capacity=capacity, sigmas=sigmas,
                         sig_min=sig_min, sig_max=sig_max, adaptive=adaptive, env=env, duel_points=duel_points,
                         duel_credit=duel_credit)
        self.fc1_tiled = self._half_tiled   # (self.Cw stays the plain channel count)

    def _rollout(self, games, net_off, ordinal0, env_seed):
        if self.duel is not None:
            from .duel_rollout import HalfDuelRollout   # (imports this module)
            return HalfDuelRollout(games, net_off, ordinal0, self.C, self.n_actions, self.slab, env_seed, self.per_gen,
                                   self.device, fc1_tiled=self._half_tiled, **self.duel)
        return HalfSynthRollout(games, net_off, ordinal0, self.C, self.n_actions, self.slab, env_seed, self.per_gen, self.device,
                                fc1_tiled=self._half_tiled)

    def _initial_distance(self, r):
        L.call("coevo_dqn16_distance", self._ptr(r, "stale"), self._ptr(r, "pop"), self.pop, self.C, self.n_actions,
               L._p(self.dist_partial))

    def _breed_children(self, ri, r, c_lo, c_hi, g):
        L.call("coevo_dqn16_perturb_dist_tiled" if self.fc1_tiled else "coevo_dqn16_perturb_dist",
               self._ptr(r, "elite"), self.parent_idx.data_ptr() + 4 * c_lo, self._ptr(r, "pop"),
               1 + c_lo, c_hi - c_lo, self.C, self.n_actions, self.sigma32.data_ptr() + 4 * ri, self.philox_seed, c_lo, ri, 0, g,
               0, self._ptr(r, "stale"), L._p(self.dist_partial))
