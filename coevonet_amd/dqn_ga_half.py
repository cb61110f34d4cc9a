"""Float16 Co-GA generations over DeepQN policies on one GPU: ``HalfDQNGAEngine``, the engine of ``args.precision ==
"float16"`` nets for the two-player Atari games (reference Atari/deepqn.py:12-37, genetic_algorithm.py:51-345), and
``HalfSynthRollout``, its rollout over the synthetic env.

The population, the Hall of Fame, the elites and the stale agent of the two roles live in ONE fp16 slab (coevo_dqn16_pack's
layout, ``DQNGAEngine``'s regions per role).  A generation is ``DQNGAEngine``'s on one rank with float16 calls: the rollout of
all 2 * pop * hof games plus the evaluation games of the previous generation's best pair (coevo_synth_step +
coevo_dqn16_forward_argmax per agent-step), then the tail - coevo_ga_select on fp16-valued distances, coevo_ga_adapt_sigma,
the gathers (coevo_net_gather with the stride in words), the offspring with their stale-agent distances fused in
(coevo_dqn16_perturb_dist, coevo_fc16_distance_finalize) and the counter tick - captured once into a hipGraph and replayed.
The rounding points are DESIGN.md 6a "Float16 DeepQN" and "Float16 DeepQN breeding".

One rank, one cohort, frames synthesised on the device.  ``DQNGATrainer`` / ``dqn_genetic_algorithm_train`` still refuse
float16: this object is the float16 route until the trainers are switched over."""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L
from .atari_synthetic import SYNTH_SEED
from .dqn_population import ROLES2, SynthRollout
from .population import N_EVAL, NetTable, SlabIO, slab_layout


class HalfSynthRollout(SynthRollout):
    """``SynthRollout``'s game and task tables (one cohort) over an fp16 slab: ``net_off`` counts 32-bit words of
    coevo_dqn16_pack's layout.  Per agent-step it enqueues coevo_synth_step (books the previous action, writes the next frames)
    and coevo_dqn16_forward_argmax; it synchronises with nothing, so a generation can be captured into a graph."""

    def __init__(self, game_nets, net_off, ordinal0, C, n_actions, slab, env_seed, ordinals_per_gen, device="cuda"):
        super().__init__(game_nets, net_off, ordinal0, C, n_actions, slab, env_seed, ordinals_per_gen, device)
        ln = self.lanes[0]
        ln["ws"] = torch.zeros(int(L.load().coevo_dqn16_workspace_bytes(ln["n"])) // 4, dtype=torch.float32, device=device)

    def start_timing(self, pairs=512, every=7):
        raise NotImplementedError("HalfSynthRollout: the float16 forward has no timed form")

    def _enqueue_lane(self, ln, T, g, stream, timed):
        m = ln["n"]
        lib = L.load()
        for t in range(T + 1):
            p, q = t & 1, (t - 1) & 1
            L._check(lib.coevo_synth_step(L._p(self.gstate), L._p(self.acc), m, L._p(self.ordinal0), g, self.ordinals_per_gen,
                                          t, L._p(self.limit), L._p(ln["rows"][q]) if t else None,
                                          ln["actions"][q].data_ptr() if t else None,
                                          L._p(ln["rows"][p]) if t < T else None, L._p(ln["frames"]) if t < T else None,
                                          self.C, self.n_actions, self.env_seed, stream), "coevo_synth_step")
            if t < T:
                L._check(lib.coevo_dqn16_forward_argmax(L._p(self.slab), L._p(ln["tasks"][p]), ln["n_tasks"][p],
                                                        ln["max_rows"][p], m, self.C, self.n_actions, L._p(ln["frames"]),
                                                        ln["actions"][p].data_ptr(), None, L._p(self.status), L._p(ln["ws"]),
                                                        stream), "coevo_dqn16_forward_argmax")

    def weight_bytes_per_round(self):
        """algorithmic bytes of one round (two agent-steps): every distinct acting fp16 weight set once per agent-step + the
        frames"""
        net_bytes = int(L.load().coevo_dqn16_slab_stride(self.C, self.n_actions)) * 4
        nets = sum(len({int(t["net_off"]) for t in tn}) for tn in self.tasks_np)
        return nets * net_bytes + 2 * self.n_games * 84 * 84 * self.C


class HalfDQNGAEngine(SlabIO):
    """Device-resident float16 population / HoF / elites of first_0 and second_0 and the generation step.

    ``load_initial`` -> ``step()`` per generation -> ``eval_only()`` for the last generation's evaluation games.  Nets go in and
    out as flat float32 arrays of fp16 values in parameters() order (``DeepQNHalf.flat()``)."""
    _pack_unpack = ("coevo_dqn16_pack", "coevo_dqn16_unpack")   # flat arrays carry fp16 values in float32

    def __init__(self, pop, hof, elites, C, n_actions, T_train, T_eval, device="cuda", env_seed=SYNTH_SEED, philox_seed=0,
                 first_ordinal=1, capacity=1024, sigmas=(0.05, 0.05), sig_min=0.001, sig_max=0.2, adaptive=True, *,
                 shard=(0, 1), gather=None, frames="device"):
        # what float16 does not cover is refused before the library is loaded
        if tuple(shard) != (0, 1):
            raise ValueError(f"HalfDQNGAEngine: precision float16 runs on one rank only, not shard {tuple(shard)}")
        if frames != "device":
            raise ValueError(f'HalfDQNGAEngine: precision float16 synthesises frames on the device only, not frames="{frames}"')
        if gather is not None:
            raise ValueError("HalfDQNGAEngine: precision float16 runs on one rank only and takes no gather")
        if not (1 <= elites <= pop and hof >= 1):
            raise ValueError(f"HalfDQNGAEngine: elites {elites} (1 .. population {pop}) or hof {hof} (>= 1) out of range")
        self.pop, self.hof, self.E, self.C, self.n_actions = pop, hof, elites, C, n_actions
        self.T_train, self.T_eval = int(T_train), int(T_eval)
        self.T = max(self.T_train, self.T_eval)
        self.device, self.philox_seed = device, int(philox_seed)
        lib = L.load()
        self.stride = int(lib.coevo_dqn16_slab_stride(C, n_actions))   # 32-bit words
        self.P = int(lib.coevo_dqn_param_count(C, n_actions))
        if self.stride <= 0:
            raise ValueError(f"HalfDQNGAEngine: {C} channels / {n_actions} actions is not a DeepQN shape")
        strides = dict.fromkeys(ROLES2, self.stride)
        self.base, total = slab_layout(ROLES2, (("pop", pop), ("hof", hof), ("elite", elites), ("stale", 1), ("hof_tmp", hof),
                                                ("elite_prev", elites)), strides)
        self.slab = torch.zeros(total, dtype=torch.int32, device=device)
        # ---- DQNGAEngine's game table: this generation's games + the evaluation games of the previous one
        net = NetTable(self.base, strides)
        h, M = hof, 2 * pop * hof
        self.per_gen = M + N_EVAL
        games, ordinal0 = [], []
        for ph, role in enumerate(ROLES2):
            for i in range(pop):
                for k in range(h):
                    opp = net("hof", ROLES2[1 - ph], h - 1 - k)
                    games.append((net("pop", role, i), opp) if ph == 0 else (opp, net("pop", role, i)))
                    ordinal0.append(first_ordinal + ph * pop * hof + i * hof + k)
        self.n_main = len(games)
        for j in range(N_EVAL):  # the best pair = the newest HoF members; generation g-1's games ride in g's launch
            games.append((net("hof", "first_0", h - 1), net("hof", "second_0", h - 1)))
            ordinal0.append(first_ordinal - self.per_gen + M + j)
        self.ro = HalfSynthRollout(games, net.net_off, ordinal0, C, n_actions, self.slab, env_seed, self.per_gen, device)
        # ---- device-resident loop state
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.gen_dev = torch.zeros(1, **i32)
        self.sigma64 = torch.tensor([sigmas[0], sigmas[1], 0.0], dtype=torch.float64, device=device)
        self.sigma32 = self.sigma64.to(torch.float32)
        self.cap = int(capacity)
        self.hist = torch.zeros(3, self.cap, dtype=torch.float64, device=device)
        self.sig_hist = torch.zeros(3, self.cap, dtype=torch.float64, device=device)
        self.loop_args = (float(sig_min), float(sig_max), 1 if adaptive else 0)
        self.dist_all = torch.zeros(2, pop, **f32)   # fp16 values in fp32 words
        self.div = [torch.zeros(1, **f32) for _ in ROLES2]
        self.fitness = [torch.zeros(pop, **f32) for _ in ROLES2]
        self.order = [torch.zeros(pop, **i32) for _ in ROLES2]
        self.best_dist = [torch.zeros(1, **f32) for _ in ROLES2]
        self.pblocks = int(lib.coevo_dqn16_perturb_blocks(C, n_actions))
        self.dist_partial = torch.zeros(max(pop, 1) * self.pblocks, dtype=torch.float64, device=device)
        self.parent_idx = torch.tensor([c % elites for c in range(max(pop - 1, 1))], **i32)
        self.iota = torch.arange(max(pop, hof, elites, 2), **i32)
        self.hof_shift_idx = torch.arange(1, max(hof, 2), **i32)
        self._graph = None
        self.generation = 0
        self.steps_per_generation = 2 * pop * hof * self.T_train + N_EVAL * self.T_eval

    # ------------------------------------------------------------------ loading weights (population.SlabIO)
    def _net_args(self, role):
        return (self.C, self.n_actions)

    def upload(self, role, region, first, flat_np):
        super().upload(role, region, first, flat_np)
        torch.cuda.current_stream().synchronize()

    def load_initial(self, pop_flat, hof_flat):
        """pop_flat[role] [pop][P], hof_flat[role] [hof][P] (rounded to fp16 on the way in); the stale agent of Q3 is the
        initial pop[pop-1]; the distances of the initial population to it (later: fused into breeding)"""
        for r in ROLES2:
            self.upload(r, "pop", 0, pop_flat[r])
            self.upload(r, "hof", 0, hof_flat[r])
            self.upload(r, "stale", 0, pop_flat[r][self.pop - 1:self.pop])
        for ri, r in enumerate(ROLES2):
            L.call("coevo_dqn16_distance", self._ptr(r, "stale"), self._ptr(r, "pop"), self.pop, self.C, self.n_actions,
                   L._p(self.dist_partial))
            L.call("coevo_fc16_distance_finalize", L._p(self.dist_partial), self.pblocks, self.pop,
                   self.dist_all[ri].data_ptr(), 0, None)
        torch.cuda.current_stream().synchronize()

    # ------------------------------------------------------------------ one generation
    def _tail(self):
        """selection -> sigma rule -> elites / HoF / best -> children + their distances -> generation counter tick:
        DQNGAEngine._tail's one-rank branch with the float16 calls"""
        ro, g = self.ro, L._p(self.gen_dev)
        roles = (L.GaSelectRole * 3)()
        for ri in range(2):
            roles[ri] = L.GaSelectRole(self.dist_all[ri].data_ptr(), L._p(ro.acc), L._p(self.div[ri]), L._p(self.fitness[ri]),
                                       L._p(self.order[ri]), L._p(self.best_dist[ri]), ri * self.pop * self.hof, ri)
        L.call("coevo_ga_select", roles, 2, self.pop, self.hof, self.hof)
        mn, mx, adaptive = self.loop_args
        L.call("coevo_ga_adapt_sigma", L._p(ro.acc), self.n_main, g, L._p(self.hist), L._p(self.sig_hist), self.cap,
               L._p(self.sigma64), L._p(self.sigma32), mn, mx, adaptive)
        for ri, r in enumerate(ROLES2):
            L.call("coevo_net_gather", self._ptr(r, "pop"), L._p(self.order[ri]), self._ptr(r, "elite"), 0, self.E, self.stride)
            if self.hof > 1:  # hof.pop(0); hof.append(best)
                L.call("coevo_net_gather", self._ptr(r, "hof"), L._p(self.hof_shift_idx), self._ptr(r, "hof_tmp"), 0,
                       self.hof - 1, self.stride)
                L.call("coevo_net_gather", self._ptr(r, "hof_tmp"), L._p(self.iota), self._ptr(r, "hof"), 0, self.hof - 1,
                       self.stride)
            L.call("coevo_net_gather", self._ptr(r, "elite"), L._p(self.iota), self._ptr(r, "hof"), self.hof - 1, 1, self.stride)
            L.call("coevo_net_gather", self._ptr(r, "elite"), L._p(self.iota), self._ptr(r, "pop"), 0, 1, self.stride)
            if self.pop > 1:   # child c = individual c + 1 from elite[c % E], noise stream (c, 4 gen + role index)
                L.call("coevo_dqn16_perturb_dist", self._ptr(r, "elite"), L._p(self.parent_idx), self._ptr(r, "pop"), 1,
                       self.pop - 1, self.C, self.n_actions, self.sigma32.data_ptr() + 4 * ri, self.philox_seed, 0, ri, 0, g, 0,
                       self._ptr(r, "stale"), L._p(self.dist_partial))
                L.call("coevo_fc16_distance_finalize", L._p(self.dist_partial), self.pblocks, self.pop - 1,
                       self.dist_all[ri].data_ptr(), 1, L._p(self.best_dist[ri]))
            else:
                self.dist_all[ri][0:1].copy_(self.best_dist[ri])
        L.call("coevo_counter_add", g, 1)

    def step(self, use_graph=True):
        gen = self.generation
        if gen >= self.cap:
            raise RuntimeError(f"generation {gen} exceeds the device history capacity ({self.cap})")
        if gen <= 1:  # the evaluation games of "generation -1" do not exist: disabled in generation 0 only
            limits = np.full(self.ro.n_games, self.T_train, dtype=np.int32)
            limits[self.n_main:] = self.T_eval if gen == 1 else 0
            self.ro.set_limits(limits)
        if use_graph:
            if self._graph is None:
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, capture_error_mode="thread_local"):
                    self.ro.enqueue(self.T, self.gen_dev)
                    self._tail()
                self._graph = gr
            self._graph.replay()
        else:
            self.ro.enqueue(self.T, self.gen_dev)
            self._tail()
        self.generation += 1

    def eval_only(self):
        """the evaluation games of the last generation (they would ride in the next one): main games disabled"""
        ro = self.ro
        limits = np.zeros(ro.n_games, dtype=np.int32)
        limits[self.n_main:] = self.T_eval
        ro.set_limits(limits)
        ro.enqueue(self.T_eval, self.gen_dev)
        torch.cuda.synchronize()
        L.raise_on_status(ro.status)
        r = ro.acc[self.n_main:].cpu().numpy()
        tot = [0.0, 0.0]
        for j in range(N_EVAL):
            for s in range(2):
                tot[s] += float(r[j, s])
        limits[:self.n_main] = self.T_train
        ro.set_limits(limits)
        return [t / 10 for t in tot]

    def close(self):
        self.ro.close()
