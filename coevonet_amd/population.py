"""What the population engines share: the slab layout, the numbering of the weight sets a rollout reads, the game tables
of Co-GA and Co-ES, the evaluation mean and gate, graph capture, the slab I/O calls, the per-generation rollout schedules, the
Co-GA generation tail of the fully connected engines, the Co-ES update of the float32 engines and the trainers' sigma rule.

GAEngine / HalfGAEngine (genetic_algorithm.py, ga_half.py), ESEngine / HalfESEngine (evolutionary_strategy.py, es_half.py)
and DQNGAEngine / HalfDQNGAEngine / DQNESEngine (dqn_population.py, dqn_ga_half.py) differ in precision, strides and kernels,
not in who plays whom: the seat rules of the reference's generation bodies are written ONCE, here.  slab_layout, NetTable,
co_ga_games, co_ga_reset_segments, co_ga_games2, co_es_games, co_es_games2, cross_games, cross_games2 (the game tables of
crossplay.py), mean_eval, eval_gate_limits, fused_tail_fits and the sigma rule are plain python - they touch neither torch
nor the library, which this module imports for captured() and the mixins only - and are pinned by
tests/test_population_cpu.py; the mixins hold the calls the engines made identically (tests/test_ga_launch_scripts_cpu.py,
tests/test_es_launch_scripts_cpu.py: recorded before they were shared).
"""
from __future__ import annotations

import ctypes as ct
import os

import numpy as np
import torch

from . import lib as L
from .rollout import DeviceRollout, RolloutPlan

ROLES = ("agent_0", "agent_1", "adversary_0")
ROLE_D = {"agent_0": 10, "agent_1": 10, "adversary_0": 8}
RET_SLOT = {"agent_0": 0, "agent_1": 1, "adversary_0": 2}    # position in play_game's return triple
ROLES2 = ("first_0", "second_0")   # the two-player Atari games (DeepQN engines)
N_EVAL = 10
ES_CHUNKS = 8   # the canonical ES summation: this many chunk sums, added left to right (include/coevo.h, K5)
SIGMA_ATTR = {"agent_0": "mutation_power_agent_0", "agent_1": "mutation_power_agent_1",
              "adversary_0": "mutation_power_adversary"}


def slab_layout(roles, regions, stride_of):
    """role after role, region after region: -> (base[role][region] in 32-bit words, slab length).  regions: ordered
    (name, count of nets); stride_of[role]: words per net"""
    base, off = {}, 0
    for r in roles:
        base[r] = {}
        for region, count in regions:
            base[r][region] = off
            off += count * stride_of[r]
    return base, off


class NetTable:
    """The weight sets a rollout reads, numbered in order of first use: table(region, role, i) -> net id; net_off[id] is the
    set's slab offset, net_D[id] its observation width (D_of = None: DeepQN, one width)."""

    def __init__(self, base, stride_of, D_of=None):
        self.base, self.stride_of, self.D_of = base, stride_of, D_of
        self.net_off, self.net_D, self.ids = [], [], {}

    def __call__(self, region, role, i=0):
        key = (region, role, i)
        if key not in self.ids:
            self.ids[key] = len(self.net_off)
            self.net_off.append(self.base[role][region] + i * self.stride_of[role])
            if self.D_of is not None:
                self.net_D.append(self.D_of[role])
        return self.ids[key]


def co_ga_games(net, lo, hi, hof):
    """One Co-GA generation launch of the individuals [lo, hi) of every role -> (games as (adversary, agent_0, agent_1) net
    ids, n_main): role by role, individual by individual, opponents from the NEWEST Hall of Fame member to the oldest (only the
    last game counts, Q2), then the N_EVAL evaluation games of the newest trio."""
    games, h = [], hof
    for role in ROLES:
        for i in range(lo, hi):
            for k in range(h):
                if role == "agent_0":      # genetic_algorithm.py:136-142
                    a0, a1, adv = net("pop", role, i), net("hof", "agent_1", h - 1 - k), net("hof", "adversary_0", h - 1 - k)
                elif role == "agent_1":    # :168-174
                    a0, a1, adv = net("hof", "agent_0", h - 1 - k), net("pop", role, i), net("hof", "adversary_0", h - 1 - k)
                else:                      # :201-207, Q4: agent_1's seat is also filled from hof_agent_0
                    a0, a1, adv = net("hof", "agent_0", h - 1 - k), net("hof", "agent_0", h - 1 - k), net("pop", role, i)
                games.append((adv, a0, a1))
    n_main = len(games)
    for _ in range(N_EVAL):  # evaluate_current_weights(best trio) = newest HoF members (:12-29, :301)
        games.append((net("hof", "adversary_0", h - 1), net("hof", "agent_0", h - 1), net("hof", "agent_1", h - 1)))
    return games, n_main


def co_ga_reset_segments(base, base_prev, pop, hof, lo, n_local, a, b, prev_eval):
    """Reset ordinals (Q6) of the games that the individuals [a, b) of a rank holding [lo, lo + n_local) play in one generation
    launch -> [(game_first, count, first_ordinal), ...]: per phase their run of the rank's table, under the ordinals from
    base (the generation's first) + ph pop hof + a hof on, whichever rank plays them.  prev_eval: + the evaluation games of
    the generation before behind the rank's main games, under the ordinals behind THAT generation's (base_prev) main games."""
    segs = [(ph * n_local * hof + (a - lo) * hof, (b - a) * hof, base + ph * pop * hof + a * hof) for ph in range(3)]
    if prev_eval:
        segs.append((3 * n_local * hof, N_EVAL, base_prev + 3 * pop * hof))
    return segs


def co_ga_games2(net, lo, hi, hof, first_ordinal, pop):
    """The two-role Co-GA generation launch of the individuals [lo, hi) of a population of `pop` -> (games as (first_0,
    second_0) net ids, the reset ordinal of each game in generation 0, n_main): phase by role, individual by individual,
    opponents from the NEWEST Hall of Fame member of the other role to the oldest; the role sits in its own seat.  Then the N_EVAL
    evaluation games of the newest pair: those of generation g - 1 ride in generation g's launch, under the ordinals behind
    that generation's main games (first_ordinal - per_gen + M + j)."""
    games, ordinal0, h, M = [], [], hof, 2 * pop * hof
    per_gen = M + N_EVAL
    for ph, role in enumerate(ROLES2):
        for i in range(lo, hi):
            for k in range(h):
                opp = net("hof", ROLES2[1 - ph], h - 1 - k)
                games.append((net("pop", role, i), opp) if ph == 0 else (opp, net("pop", role, i)))
                ordinal0.append(first_ordinal + ph * pop * hof + i * hof + k)
    n_main = len(games)
    for j in range(N_EVAL):
        games.append((net("hof", "first_0", h - 1), net("hof", "second_0", h - 1)))
        ordinal0.append(first_ordinal - per_gen + M + j)
    return games, ordinal0, n_main


def co_es_games(net, n):
    """One Co-ES generation of n individuals -> (games, eval_games): game 3j + role seats perturbed net j of the role against
    the two other base nets; the N_EVAL evaluation games seat the base trio."""
    games = []
    for j in range(n):  # evolutionary_strategy.py:236-251: mutate_weights for agent_0, agent_1, adversary_0
        for r in ROLES:
            seat = {q: net("base", q) for q in ROLES}
            seat[r] = net("pert", r, j)
            games.append((seat["adversary_0"], seat["agent_0"], seat["agent_1"]))
    # Unlike Co-GA, the evaluation games cannot ride in the next generation's launch: they play the UPDATED base nets, and
    # generation g+1 perturbs with sigma_{g+1}, which the adaptive rule derives from generation g's evaluation
    # (evolutionary_strategy.py:272-316).  They get their own 10-game rollout after each update.
    eval_games = [(net("base", "adversary_0"), net("base", "agent_0"), net("base", "agent_1"))] * N_EVAL
    return games, eval_games


def co_es_games2(net, lo, hi, first_ordinal, pop):
    """The two-role Co-ES generation of the individuals [lo, hi) of a population of `pop` -> (games as (first_0, second_0)
    net ids, the reset ordinal of each game in generation 0, the N_EVAL evaluation games of the base pair, their ordinals):
    the two base nets are numbered first, then game 2j + role seats perturbed net j of the role (rank-local slab index
    j - lo; ordinal first_ordinal + 2j + role, whichever shard plays it) against the other role's base net; the evaluation
    games take the ordinals behind the population's main games."""
    base = [net("base", r) for r in ROLES2]
    games, ordinal0 = [], []
    for j in range(lo, hi):
        for ri, r in enumerate(ROLES2):
            me = net("pert", r, j - lo)
            games.append((me, base[1]) if ri == 0 else (base[0], me))
            ordinal0.append(first_ordinal + 2 * j + ri)
    return games, ordinal0, [tuple(base)] * N_EVAL, [first_ordinal + 2 * pop + j for j in range(N_EVAL)]


def cross_games(net, A, B, C, E):
    """A cross-play of A agent_0 x B agent_1 x C adversary nets, E episodes per trio -> (games as (adversary, agent_0, agent_1)
    net ids, episode of each game): game ((a B + b) C + c) E + e seats (adversary c, agent_0 a, agent_1 b) in episode e.  The
    reset ordinal of a game is first_ordinal + its episode: every trio meets the same E initial worlds."""
    games, episode = [], []
    for a in range(A):
        for b in range(B):
            for c in range(C):
                seat = (net("cross", "adversary_0", c), net("cross", "agent_0", a), net("cross", "agent_1", b))
                for e in range(E):
                    games.append(seat)
                    episode.append(e)
    return games, episode


def cross_games2(net, A, B, E):
    """The two-player twin: game (a B + b) E + e seats (first_0 a, second_0 b) in episode e -> (games, episode of each game)"""
    games, episode = [], []
    for a in range(A):
        for b in range(B):
            seat = (net("cross", "first_0", a), net("cross", "second_0", b))
            for e in range(E):
                games.append(seat)
                episode.append(e)
    return games, episode


def mean_eval(rewards, n_slots):
    """mean reward per slot of the N_EVAL evaluation games rewards[g][slot]"""
    tot = [0.0] * n_slots
    for g in range(N_EVAL):  # python-float accumulation order of evaluate_current_weights
        for s in range(n_slots):
            tot[s] += float(rewards[g, s])
    return [t / 10 for t in tot]


def mean_eval_triple(rewards):
    """mean reward triple (agent_0, agent_1, adversary_0) of the N_EVAL evaluation games rewards[g][slot]"""
    return mean_eval(rewards, 3)


def eval_gate_limits(n_games, n_main, T_train, T_eval, gen):
    """step limits of generation `gen`'s launch: the main games play T_train steps; the evaluation games riding along are
    those of generation gen - 1, which do not exist in generation 0 (limit 0: disabled)"""
    limits = np.full(n_games, T_train, dtype=np.int32)
    limits[n_main:] = T_eval if gen > 0 else 0
    return limits


def captured(fn):
    """fn()'s launches as a graph: captured on the current stream, nothing executed"""
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        fn()
    return gr


def _per_role(v, role):
    """the fully connected engines keep stride / P per role, the DeepQN engines one number"""
    return v[role] if isinstance(v, dict) else v


class SlabIO:
    """Nets in and out of ``self.slab`` as flat float32 arrays [n][P] in parameters() order.  A class names its (pack, unpack)
    entry points in ``_pack_unpack`` and their trailing arguments in ``_net_args``."""
    _pack_unpack = ("coevo_fc_pack", "coevo_fc_unpack")

    def _net_args(self, role):
        return (ROLE_D[role],)

    def _uploaded(self, region):
        """what an upload into `region` invalidates"""

    def _ptr(self, role, region, i=0):
        return self.slab.data_ptr() + 4 * (self.base[role][region] + i * _per_role(self.stride, role))

    def upload(self, role, region, first, flat_np):
        """flat_np [n][P] -> nets first.. of a region"""
        flat = torch.from_numpy(np.ascontiguousarray(flat_np, dtype=np.float32)).to(self.device)
        L.call(self._pack_unpack[0], L._p(flat), self._ptr(role, region, first), flat.shape[0], *self._net_args(role))
        self._uploaded(region)
        return flat  # keep alive until the stream has consumed it

    def download(self, role, region, first, n):
        out = torch.zeros(n, _per_role(self.P, role), dtype=torch.float32, device=self.device)
        L.call(self._pack_unpack[1], self._ptr(role, region, first), L._p(out), n, *self._net_args(role))
        return out.cpu().numpy()


def _host(rewards):
    return rewards.cpu().numpy() if torch.is_tensor(rewards) else rewards


class CoGASchedule:
    """Which games of the Co-GA table play when, and under which reset ordinals (Q6: one seeded stream addressed by game
    ordinal).  Needs pop, hof, lo, n_local, n_main, first_ordinal, T_train, T_eval, n_cycles, env_mode, plan, ro."""
    # True: the whole population is here (lo = 0, n_local = pop), so the three phases are ONE run of game ordinals and take one
    # reset launch (HalfGAEngine).  GAEngine keeps its launch per phase, whole population or shard.
    one_reset = False

    def load_initial(self, pop_flat, hof_flat):
        """pop_flat[role] [pop][P], hof_flat[role] [hof][P]; the stale agent of Q3 is the initial pop[pop-1]"""
        keep = []
        for r in ROLES:
            keep.append(self.upload(r, "pop", 0, pop_flat[r]))
            keep.append(self.upload(r, "hof", 0, hof_flat[r]))
            keep.append(self.upload(r, "stale", 0, pop_flat[r][self.pop - 1:self.pop]))
        torch.cuda.current_stream().synchronize()

    def _ordinal_base(self, gen):
        return self.first_ordinal + gen * (3 * self.pop * self.hof + N_EVAL)

    def _reset_segments(self, gen, a, b, prev_eval):
        return co_ga_reset_segments(self._ordinal_base(gen), self._ordinal_base(gen - 1), self.pop, self.hof, self.lo,
                                    self.n_local, a, b, prev_eval)

    def rollout(self, gen, with_prev_eval):
        """plays generation `gen`'s 3*n_local*hof games and, riding along, the 10 evaluation games of gen-1 (they depend only on
        that generation's selection)"""
        self.ro.set_limits(eval_gate_limits(self.plan.n_games, self.n_main, self.T_train, self.T_eval, 1 if with_prev_eval else 0))
        segs = self._reset_segments(gen, self.lo, self.lo + self.n_local, with_prev_eval)
        if self.one_reset:   # (the three phases are one run of ordinals)
            assert self.n_local == self.pop
            segs = [(0, self.n_main, segs[0][2])] + segs[3:]
        self._reset(segs)
        self.ro.run(self.n_cycles)

    def _reset(self, segs):
        """the device env: a launch per segment; the host env: the ordinal of every game (0 for the others)"""
        if self.env_mode == "device":
            for seg in segs:
                self.ro.reset(*seg)
            return
        ords = np.zeros(self.plan.n_games, dtype=np.int64)
        for first, n, ordinal in segs:
            ords[first:first + n] = ordinal + np.arange(n)
        self.ro.reset_from_ordinals(ords)

    def eval_only(self, gen):
        """flush: the evaluation games of generation `gen` alone (main games disabled) -> their mean triple"""
        ro = self.ro
        ro.set_limits(eval_gate_limits(self.plan.n_games, self.n_main, 0, self.T_eval, 1))
        if self.env_mode == "device":
            ro.reset(0, self.n_main, 0)
        self._reset(self._reset_segments(gen + 1, self.lo, self.lo, True)[3:])   # (as generation gen + 1's launch would)
        ro.run((self.T_eval + 2) // 3)
        return self.eval_rewards()

    def rewards_host(self):
        return _host(self.ro.rewards)

    def eval_rewards(self):
        """mean reward triple (agent_0, agent_1, adversary_0) of the 10 evaluation games in the last rollout"""
        self.ro.check_status()
        return mean_eval_triple(self.rewards_host()[self.n_main:])

    def elite_ids(self):
        return {r: self.order[r][:self.E].cpu().numpy().astype(int).tolist() for r in ROLES}


FUSED_MAX_POP, FUSED_MAX_HOF, FUSED_MAX_E = 4096, 16, 8


def fused_tail_fits(pop, hof, elites):
    """what the fused tail's launches take: coevo_ga_select ranks the population in one workgroup (select.hip), the promotion
    launches unroll over the Hall of Fame and the elites (promote_roles.hip.h PROMOTE_MAX_HOF, PROMOTE_MAX_E)"""
    return pop <= FUSED_MAX_POP and hof <= FUSED_MAX_HOF and elites <= FUSED_MAX_E


class CoGATail:
    """The generation tail of the fully connected Co-GA engines after the rollout: selection, promotion (elites, Hall of Fame,
    best), children with their stale-agent distances - each launch sequence written once, in its fused form (one launch for
    the three roles: fused_tail_fits) and its launch-per-step form.  A class names its promotion, child and distance-reduction
    entry points and the job struct and entry points of the multi-role breeding.  Needs pop, hof, E, philox_seed, slab / base /
    stride (SlabIO._ptr), dist, div, fitness, order, best_dist, dist_partial, pblocks, parent_idx and, for the launch-per-step
    forms, iota and hof_shift_idx; for the extension modes hof_mean / population_sharing, device and _stale_distances(roles)."""
    _promote_entry = "coevo_ga_promote"
    _perturb_dist_entry = "coevo_fc_perturb_dist"
    _finalize_entry = "coevo_fc_distance_finalize"
    _perturb_job = "PerturbJob"
    _perturb_multi_entry = "coevo_fc_perturb_dist_multi"
    _finalize_multi_entry = "coevo_fc_distance_finalize_multi"
    _pairwise_entry = "coevo_fc_pairwise_distance"                  # population_sharing: all pairwise distances
    _pairwise_scratch_entry = "coevo_fc_pairwise_scratch_doubles"
    _hof_tiled = False   # (GAEngine may turn it on: the Hall of Fame then has tile-major W2 twins that the rollout reads)

    def _select_role_block(self, rewards_ptr_of, game_first_of, gathered=False):
        """GaSelectRole[3]; gathered: distances and rewards come out of the all-gathered buffer, not from these"""
        roles = (L.GaSelectRole * 3)()
        for ri, r in enumerate(ROLES):
            roles[ri] = L.GaSelectRole(None if gathered else L._p(self.dist[r]), None if gathered else rewards_ptr_of(ri),
                                       L._p(self.div[r]), L._p(self.fitness[r]), L._p(self.order[r]), L._p(self.best_dist[r]),
                                       0 if gathered else game_first_of(ri), RET_SLOT[r])
        return roles

    def _select_roles(self, rewards_ptr_of, game_first_of, games_per_individual):
        L.call("coevo_ga_select", self._select_role_block(rewards_ptr_of, game_first_of), 3, self.pop, games_per_individual,
               self.hof)

    def _select_unfused(self, rewards_ptr_of, game_first_of, games_per_individual):
        for ri, r in enumerate(ROLES):
            L.call("coevo_sharing_score", L._p(self.dist[r]), self.pop, L._p(self.div[r]))
            L.call("coevo_ga_fitness", rewards_ptr_of(ri), game_first_of(ri), self.pop, games_per_individual, self.hof,
                   RET_SLOT[r], L._p(self.div[r]), L._p(self.fitness[r]))
            L.call("coevo_rank_desc", L._p(self.fitness[r]), self.pop, L._p(self.order[r]))

    def _promote_roles(self, elites_from_pop, best_to_pop0, tick=False, rebuild=None):
        """elites (out of the population, or - rebuild = (noise stream base, device generation or None) - rebuilt from last
        generation's elites and the noise their children were bred with), Hall of Fame FIFO and the best to pop[0] in one
        launch; tick: + the generation counter's increment, the last launch of the generation's tail"""
        roles = (L.GaPromoteRole * 3)()
        for ri, r in enumerate(ROLES):
            roles[ri] = L.GaPromoteRole(self._ptr(r, "pop"), self._ptr(r, "hof"), self._ptr(r, "elite"),
                                        L._p(self.order[r]), ROLE_D[r], 1 if elites_from_pop else 0,
                                        1 if best_to_pop0 else 0, 0)
        tiled = self._hof_tiled
        if tick and rebuild is None and tiled:
            L.call("coevo_ga_promote_tick_tiled", roles, 3, self.E, self.hof, L._p(self.gen_dev), L._p(self.hof_twin))
            return
        if rebuild is not None:
            L.call("coevo_ga_promote_rebuild", roles, 3, self.E, self.hof, L._p(self.sigma32_prev), self.philox_seed, *rebuild)
        elif tick:
            L.call("coevo_ga_promote_tick", roles, 3, self.E, self.hof, L._p(self.gen_dev))
        else:
            L.call(self._promote_entry, roles, 3, self.E, self.hof)
        if tiled:
            self._refresh_hof_twins()

    def _elites_unfused(self, r, rebuild=None):
        """the elites of role r out of the population slab or - rebuild = (sigma pointer, noise stream, device generation or
        None): a rank that holds only its own children - from last generation's elites and the counter-based noise"""
        D = ROLE_D[r]
        if rebuild is None:
            L.call("coevo_fc_gather", self._ptr(r, "pop"), L._p(self.order[r]), self._ptr(r, "elite"), 0, self.E, D)
            return
        sigma_ptr, stream, gen_ptr = rebuild
        L.call("coevo_fc_gather", self._ptr(r, "elite"), L._p(self.iota), self._ptr(r, "elite_prev"), 0, self.E, D)
        L.call("coevo_fc_rebuild_elites", self._ptr(r, "elite_prev"), L._p(self.order[r]), self._ptr(r, "elite"), self.E, D,
               sigma_ptr, self.philox_seed, stream, gen_ptr)

    def _hof_push(self, r):
        """hof.append(best); hof.pop(0)  (genetic_algorithm.py:270-275)"""
        D = ROLE_D[r]
        if self.hof > 1:
            L.call("coevo_fc_gather", self._ptr(r, "hof"), L._p(self.hof_shift_idx), self._ptr(r, "hof_tmp"), 0,
                   self.hof - 1, D)
            L.call("coevo_fc_gather", self._ptr(r, "hof_tmp"), L._p(self.iota), self._ptr(r, "hof"), 0,
                   self.hof - 1, D)
        L.call("coevo_fc_gather", self._ptr(r, "elite"), L._p(self.iota), self._ptr(r, "hof"), self.hof - 1, 1, D)
        if self._hof_tiled:
            self._refresh_hof_twins()

    def _best_to_pop0(self, r):
        L.call("coevo_fc_gather", self._ptr(r, "elite"), L._p(self.iota), self._ptr(r, "pop"), 0, 1, ROLE_D[r])

    def _promote_unfused(self, r, best_to_pop0=True, best_dist=False):
        """behind the elites of role r: Hall of Fame FIFO, [the best to pop[0]], [the best's own stale-agent distance]"""
        self._hof_push(r)
        if best_to_pop0:
            self._best_to_pop0(r)
        if best_dist:
            L.call("coevo_gather_f32", L._p(self.best_dist[r]), L._p(self.dist[r]), L._p(self.order[r]), 1)

    def _breed_role_children(self, ri, r, c_lo, c_hi, stream, gen_dev, sigma_ptr):
        """children [c_lo, c_hi) of role r (child c = individual c + 1 from elite[c % E], noise stream (c, `stream`) - plus
        4 x the device generation, given gen_dev) and, accumulated while they are written, their stale-agent distances (Q3);
        individual 0 is the unchanged best, whose distance is the one it had"""
        L.call(self._perturb_dist_entry, self._ptr(r, "elite"), self.parent_idx.data_ptr() + 4 * c_lo, self._ptr(r, "pop"),
               1 + c_lo, c_hi - c_lo, ROLE_D[r], sigma_ptr, self.philox_seed, c_lo, stream, 0, gen_dev, self._ptr(r, "stale"),
               L._p(self.dist_partial[r]))
        L.call(self._finalize_entry, L._p(self.dist_partial[r]), self.pblocks[r], c_hi - c_lo, L._p(self.dist[r]), 1 + c_lo,
               L._p(self.best_dist[r]) if c_lo == 0 else None)

    def _breed_children_multi(self, c_lo, c_hi, sigma_ptrs, streams, gen_dev=None, tick=None):
        """_breed_role_children of the three roles as one job each of the two multi launches: sigma_ptrs[ri], streams[ri] per
        role; tick: the device counter that the distance reduction increments (a generation's last launch)"""
        Job = getattr(L, self._perturb_job)
        pj, fj = (Job * 3)(), (L.FinalizeJob * 3)()
        for ri, r in enumerate(ROLES):
            part = self.dist_partial[r].data_ptr() + 8 * c_lo * self.pblocks[r]
            pj[ri] = Job(self._ptr(r, "elite"), self.parent_idx.data_ptr() + 4 * c_lo, self._ptr(r, "pop"), sigma_ptrs[ri],
                         self._ptr(r, "stale"), part, 1 + c_lo, c_hi - c_lo, ROLE_D[r], c_lo, streams[ri], 0)
            fj[ri] = L.FinalizeJob(part, self.dist[r].data_ptr(), self.best_dist[r].data_ptr() if c_lo == 0 else None,
                                   self.pblocks[r], c_hi - c_lo, 1 + c_lo, 0)
        L.call(self._perturb_multi_entry, ct.cast(pj, ct.c_void_p), 3, self.philox_seed, 0, gen_dev)
        if tick is not None:
            L.call(self._finalize_multi_entry + "_tick", ct.cast(fj, ct.c_void_p), 3, tick)
        else:
            L.call(self._finalize_multi_entry, ct.cast(fj, ct.c_void_p), 3)

    # ---- the Co-GA extension modes hof_mean / population_sharing: one rank, the whole population here
    def _sharing_buffers(self):
        """population_sharing: all pairwise distances [pop][pop] and the niche counts [pop] of every role and the scratch
        of the pairwise launch - this mode's only buffers"""
        f32 = dict(dtype=torch.float32, device=self.device)
        self.pair_dist = {r: torch.zeros(self.pop, self.pop, **f32) for r in ROLES}
        self.niche = {r: torch.zeros(self.pop, **f32) for r in ROLES}
        n_scratch = max(int(getattr(L.load(), self._pairwise_scratch_entry)(self.pop, ROLE_D[r])) for r in ROLES)
        self.pair_scratch = torch.zeros(n_scratch, dtype=torch.float64, device=self.device)

    def _select_shared(self, rewards_ptr, per_phase):
        """select() under hof_mean / population_sharing, launch per step and role: the stale-agent distances where they are
        not current (_stale_distances), the share - niche counts over all pairwise distances, or today's score against the
        stale agent -, the fitness with the mode's switches, the ranking, and the best individual's stale-agent distance,
        which the promotion hands to the children's distances: the stale-agent chain stays valid in either mode"""
        flags =((L.K_SH["COEVO_FIT_HOF_MEAN"] if self.hof_mean else 0)
                 | (L.K_SH["COEVO_FIT_PER_INDIVIDUAL"] if self.population_sharing else 0))
        for ri, r in enumerate(ROLES):
            D = ROLE_D[r]
            self._stale_distances((r,))
            if self.population_sharing:
                L.call(self._pairwise_entry, self._ptr(r, "pop"), self.pop, D, L._p(self.pair_scratch), L._p(self.pair_dist[r]))
                L.call("coevo_niche_counts", L._p(self.pair_dist[r]), self.pop, L._p(self.niche[r]))
                share = self.niche[r]
            else:
                L.call("coevo_sharing_score", L._p(self.dist[r]), self.pop, L._p(self.div[r]))
                share = self.div[r]
            L.call("coevo_ga_fitness_shared", rewards_ptr, ri * per_phase, self.pop, self.hof, self.hof, RET_SLOT[r], flags,
                   L._p(share), L._p(self.fitness[r]))
            L.call("coevo_rank_desc", L._p(self.fitness[r]), self.pop, L._p(self.order[r]))
            L.call("coevo_gather_f32", L._p(self.best_dist[r]), L._p(self.dist[r]), L._p(self.order[r]), 1)

    def mean_niche(self):
        """per role the fp64 mean of the niche counts, computed on the host (population_sharing)"""
        return [float(np.mean(self.niche[r].cpu().numpy().astype(np.float64))) for r in ROLES]


class CoESSchedule:
    """The Co-ES training and evaluation rollouts of one generation (game ordinal 3j + role, then the evaluation games).
    Needs pop, lo, n_main, first_ordinal, T_train, T_eval, env_mode, slab, device; _rollout_pair gives plan, ro, eval_ro."""

    def _rollout_pair(self, games, eval_games, table, env_seed, cls=DeviceRollout, host_cohorts=None, **ro_kw):
        """plan / ro and eval_plan / eval_ro over self.slab.  Device env: 2 cohorts (COEVO_ES_COHORTS; 114 vs 109 generations/s
        at cfg3).  host_cohorts (env on the host cores): that many alternating cohorts of contiguous game ranges (a core then owns
        whole cache lines of the struct-of-arrays game state), rows numbered cohort by cohort (one observation / action range)."""
        cohorts = int(os.environ.get("COEVO_ES_COHORTS", "2")) if host_cohorts is None else host_cohorts
        game_cohort = None
        if host_cohorts is not None and cohorts > 1 and len(games) >= cohorts:
            game_cohort = (np.arange(len(games)) * cohorts // len(games)).astype(np.int32)
        self.plan = RolloutPlan(np.array(games), table.net_off, table.net_D, device=self.device,
                                heavy_rows=int(os.environ.get("COEVO_HEAVY_ROWS", "32")), n_cohorts=cohorts,
                                game_cohort=game_cohort, row_order="class" if host_cohorts is None else "cohort")
        self.ro = cls(self.plan, self.slab, env_seed=env_seed, **ro_kw)
        # the 10 evaluation games: three nets x 10 rows, as two 5-row streaming tasks per net (1.0 -> 0.5 ms)
        self.eval_plan = RolloutPlan(np.array(eval_games), table.net_off, table.net_D, device=self.device, split_rows=5)
        self.eval_ro = cls(self.eval_plan, self.slab, env_seed=env_seed, **ro_kw)

    def _ordinal_base(self, gen):
        return self.first_ordinal + gen * (3 * self.pop + N_EVAL)

    def rollout(self, gen):
        """this rank's 3*n_local training games of generation `gen` (game ordinal 3j + role in the seeded stream)"""
        ro = self.ro
        ro.set_limits(np.full(self.plan.n_games, self.T_train, dtype=np.int32))
        first = self._ordinal_base(gen) + 3 * self.lo
        if self.env_mode == "device":
            ro.reset(0, self.n_main, first)
        else:
            ro.reset_from_ordinals(first + np.arange(self.n_main))
        if getattr(ro, "n_cohorts", 1) > 1:
            ro.enqueue((self.T_train + 2) // 3)  # cohort chains overlap only when enqueued eagerly
        else:
            ro.run((self.T_train + 2) // 3)

    def evaluate(self, gen):
        """evaluate_current_weights: 10 games of the current base trio -> mean reward triple (:22-59, :272)"""
        ro = self.eval_ro
        ro.set_limits(np.full(N_EVAL, self.T_eval, dtype=np.int32))
        first = self._ordinal_base(gen) + 3 * self.pop
        if self.env_mode == "device":
            ro.reset(0, N_EVAL, first)
        else:
            ro.reset_from_ordinals(first + np.arange(N_EVAL))
        ro.run((self.T_eval + 2) // 3)
        ro.check_status()
        return mean_eval_triple(_host(ro.rewards))

    def rewards_host(self):
        return _host(self.ro.rewards)


class CoESUpdate:
    """The Co-ES update of the float32 engines after the training rollout, written once: rewards (and distances) into ``stats``,
    gathered; per role the fitness and the chunk partial sums of the update, gathered; per role the update applied.  A class
    names its roles, its partial-sum and apply entry points (their shape arguments: SlabIO._net_args), whether its buffers per
    role (raw, fitness, div, sigma) are indexed by role or ``_by_number`` and, where the distances are not in ``stats`` by then,
    ``_local_distances``.  Also written once: the shard range with its refusals and the partial-sum layout."""
    _roles, _by_number = ROLES, False
    _partial_entry, _apply_entry = "coevo_es_partial", "coevo_es_apply"

    def _shard_range(self, pop, shard, gather, chunks, antithetic, centered_rank, rng="device_philox"):
        """this rank's individuals [lo, hi), after refusing what a Co-ES engine cannot shard or pair"""
        self.pop, self.gather, (self.rank, self.world) = pop, gather, shard
        self.antithetic, self.centered_rank, self.chunks = bool(antithetic), bool(centered_rank), int(chunks)
        if self.world > 1 and (pop % self.world or self.chunks % self.world):
            raise ValueError(f"population {pop} and the {self.chunks} update chunks must both be divisible by the "
                             f"number of ranks {self.world}")
        if (self.antithetic or self.centered_rank or self.world > 1) and rng != "device_philox":
            raise ValueError("the extension mode and the sharded run need device_philox offspring")
        if self.antithetic and pop % 2:
            raise ValueError("antithetic pairs need an even population")
        self.lo, self.hi = self.rank * pop // self.world, (self.rank + 1) * pop // self.world
        self.n_local = self.hi - self.lo

    def _partial_layout(self):
        """chunk partial sums of the update, rank-major: [world][role][chunks/world][stride_role]"""
        self.chunks_local = self.chunks // self.world
        self.part_off, o = {}, 0
        for r in self._roles:
            self.part_off[r] = o
            o += self.chunks_local * _per_role(self.stride, r)
        self.part_block = o
        self.partials = torch.zeros(self.world * self.part_block, dtype=torch.float32, device=self.device)

    def _local_distances(self):
        """this rank's distances to the base nets into stats[:, lo:hi, 1], where they are not there yet"""

    def co_es_update(self, rewards, lr, fitness_sharing):
        """compute_weight_update (evolutionary_strategy.py:120-148) + base += update on the device, from rewards [role][n_local].
        Sharded: the (reward, distance) pairs, then the chunk partial sums are all-gathered; every rank applies the same update."""
        self.stats[:, self.lo:self.hi, 0] = rewards
        if fitness_sharing:
            self._local_distances()
        if self.world > 1:
            self.gather(self, "stats")
        for ri, r in enumerate(self._roles):
            k = ri if self._by_number else r
            raw, fitness, div = self.raw[k], self.fitness[k], self.div[k]
            raw.copy_(self.stats[ri, :, 0])                  # np.array(rewards, dtype=float32)
            if fitness_sharing:
                d = self.stats[ri, :, 1].to(torch.float32).contiguous()
                L.call("coevo_sharing_score", L._p(d), self.pop, L._p(div))
                raw.div_(1.0 + div)
            if self.centered_rank:
                L.call("coevo_centered_ranks", L._p(raw), self.pop, L._p(fitness))
            else:
                fitness.copy_(raw)
            L.call(self._partial_entry, self._ptr(r, "base"), self._ptr(r, "pert"), self.lo, *self._net_args(r), L._p(fitness),
                   self.pop, self.chunks, self.rank * self.chunks_local, self.chunks_local,
                   self.partials.data_ptr() + 4 * (self.rank * self.part_block + self.part_off[r]))
        if self.world > 1:
            self.gather(self, "partials")
        for ri, r in enumerate(self._roles):
            L.call(self._apply_entry, self._ptr(r, "base"), self.partials.data_ptr() + 4 * self.part_off[r], self.chunks,
                   self.chunks_local, self.part_block, *self._net_args(r), self.pop,
                   L._p(self.sigma[ri if self._by_number else r]), L.C.c_float(lr))


# ---- what the trainers share
def adapt_mutation_power(args, gen, hist):
    """genetic_algorithm.py:323-345 (evolutionary_strategy.py:292-316 is identical): a role whose last 10 evaluation means are
    worse than the 10 before them grows its sigma, any other shrinks it; quirk Q5: agent_0 grows from agent_1's sigma."""
    for role, grows_from in (("agent_0", "agent_1"), ("agent_1", "agent_1"), ("adversary_0", "adversary_0")):
        h, attr = hist[role], SIGMA_ATTR[role]
        if gen > 10 and np.mean(h[-10:]) < np.mean(h[-20:-10]):
            setattr(args, attr, min(getattr(args, SIGMA_ATTR[grows_from]) * 1.2, args.max_mutation_power))
        else:
            setattr(args, attr, max(getattr(args, attr) * 0.95, args.min_mutation_power))


def adapt_mutation_power2(args, gen, rewards, zero_adversary):
    """the sigma rule over the two-player games: first_0 takes agent_0's part, second_0 agent_1's, a history of zeros the
    adversary's, whose sigma comes back as it was.  zero_adversary: the rule sees 0.0, not the caller's value (then required)"""
    keep = getattr(args, "mutation_power_adversary", 0.0)
    h = {"agent_0": rewards["first_0"], "agent_1": rewards["second_0"], "adversary_0": [0.0] * len(rewards["first_0"])}
    if zero_adversary:
        args.mutation_power_adversary = 0.0
    adapt_mutation_power(args, gen, h)
    args.mutation_power_adversary = keep


def shard_and_gather(dist_ctx, name):
    """-> (shard, gather callback `name` of the context): one rank without a context or in a world of one"""
    if dist_ctx is not None and dist_ctx.world > 1:
        return (dist_ctx.rank, dist_ctx.world), getattr(dist_ctx, name)
    return (0, 1), None


def _wants_half(args):
    """False for float32 (or no precision attribute), True for float16, ValueError for anything else"""
    precision = getattr(args, "precision", "float32")
    if precision == "float32":
        return False
    if precision != "float16":
        raise ValueError(f"Unsupported precision: {precision}")
    return True


def _half_one_rank_plain(args, what, dist_ctx, gather_name, extensions):
    """the refusals every float16 trainer shares: more than one rank, an extension mode"""
    shard, gather = shard_and_gather(dist_ctx, gather_name)
    if shard != (0, 1) or gather is not None:
        raise ValueError(f"{what} float16 runs on one rank only, not shard {shard}")
    for attr in extensions:
        if getattr(args, attr, False):
            raise ValueError(f"{what} float16 is not built with args.{attr}")


GA_SHARING_MODES = ("coevo_hof_mean", "coevo_population_sharing")   # Co-GA extension modes of the fully connected engine


def refuse_ga_sharing_modes(args, what):
    """the DeepQN trainers have neither mode: named, not ignored"""
    for attr in GA_SHARING_MODES:
        if getattr(args, attr, False):
            raise ValueError(f"{what} is not built with args.{attr}")


def refuse_gauntlet(args, what):
    """args.coevo_gauntlet (gauntlet.py) is served by the float32 Co-GA trainer of simple_adversary alone; the first thing the
    other trainers do"""
    if getattr(args, "coevo_gauntlet", None) is not None:
        raise ValueError(f"args.coevo_gauntlet: the baseline gauntlet is not built for {what} (only for GATrainer in float32 on "
                         "one rank, in the host-driven loop, with the device env)")


def half_route(args, what, rng, env_mode, dist_ctx, gather_name, extensions=()):
    """Which engines a trainer of the fully connected nets builds: False = the float32 ones, True = the float16 ones
    (HalfGAEngine / HalfESEngine).  What float16 does not cover is refused here with "`what` float16 ...", the first thing a
    trainer does: no other attribute of `args` has been read and the library is not loaded.  A bit-exact host_reference mode
    cannot exist in float16 (the fp16 forward rounds in the canonical order, not in torch's half BLAS order), so the route
    is rng "device_philox" + the device env on one rank, without the extension modes named in `extensions`."""
    if not _wants_half(args):
        return False
    rng = rng or getattr(args, "coevo_rng", "host_reference")
    env_mode = env_mode or getattr(args, "coevo_env", "device")
    if rng != "device_philox":
        raise ValueError(f'{what} float16 needs rng="device_philox" (the argument, or args.coevo_rng), not "{rng}": there is '
                         "no bit-exact reference mode in float16")
    if env_mode != "device":
        raise ValueError(f'{what} float16 has the device env only, not env "{env_mode}"')
    _half_one_rank_plain(args, what, dist_ctx, gather_name, extensions)
    return True


def dqn_half_route(args, what, frames_mode, dist_ctx, gather_name, extensions=()):
    """half_route for the DeepQN trainers, whose noise is always counter-based and whose env is always the synthetic one on the
    device: False = DQNGAEngine / DQNESEngine, True = HalfDQNGAEngine / HalfDQNESEngine.  Refused with "`what` float16 ...":
    frames rendered on the host (``frames_mode(args)``: args.coevo_frames / COEVO_DQN_FRAMES), more than one rank, the
    extension modes named in `extensions`.  The first thing a trainer does, as above."""
    if not _wants_half(args):
        return False
    if frames_mode(args) != "device":
        raise ValueError(f'{what} float16 synthesises frames on the device only, not frames "{frames_mode(args)}"')
    _half_one_rank_plain(args, what, dist_ctx, gather_name, extensions)
    return True
