"""What the population engines share: the slab layout, the numbering of the weight sets a rollout reads, the game tables
of Co-GA and Co-ES, the evaluation mean and gate, graph capture, the slab I/O calls, the per-generation rollout schedules and
the Co-GA generation tail of the fully connected engines.

GAEngine / HalfGAEngine (genetic_algorithm.py, ga_half.py), ESEngine / HalfESEngine (evolutionary_strategy.py, es_half.py)
and DQNGAEngine / HalfDQNGAEngine / DQNESEngine (dqn_population.py, dqn_ga_half.py) differ in precision, strides and kernels,
not in who plays whom: the seat rules of the reference's generation bodies are written ONCE, here.  slab_layout, NetTable,
co_ga_games, co_ga_games2, co_es_games, mean_eval and eval_gate_limits are plain python - they touch neither torch nor the
library, which this module imports for captured() and the mixins only - and are pinned by tests/test_population_cpu.py; the
mixins hold the calls the engines made identically (tests/test_ga_launch_scripts_cpu.py: recorded before they were shared).
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L

ROLES = ("agent_0", "agent_1", "adversary_0")
ROLE_D = {"agent_0": 10, "agent_1": 10, "adversary_0": 8}
RET_SLOT = {"agent_0": 0, "agent_1": 1, "adversary_0": 2}    # position in play_game's return triple
ROLES2 = ("first_0", "second_0")   # the two-player Atari games (DeepQN engines)
N_EVAL = 10


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

    def rollout(self, gen, with_prev_eval):
        """plays generation `gen`'s 3*n_local*hof games and, riding along, the 10 evaluation games of gen-1 (they depend only on
        that generation's selection)"""
        ro, M = self.ro, 3 * self.pop * self.hof
        ro.set_limits(eval_gate_limits(self.plan.n_games, self.n_main, self.T_train, self.T_eval, 1 if with_prev_eval else 0))
        base = self._ordinal_base(gen)
        per_phase = self.n_local * self.hof
        if self.env_mode == "device":
            if self.one_reset:
                assert self.n_local == self.pop
                ro.reset(0, self.n_main, base)
            else:
                for ph in range(3):
                    ro.reset(ph * per_phase, per_phase, base + ph * self.pop * self.hof + self.lo * self.hof)
            if with_prev_eval:
                ro.reset(self.n_main, N_EVAL, self._ordinal_base(gen - 1) + M)
        else:
            ords = np.zeros(self.plan.n_games, dtype=np.int64)
            for ph in range(3):
                ords[ph * per_phase:(ph + 1) * per_phase] = (base + ph * self.pop * self.hof + self.lo * self.hof
                                                             + np.arange(per_phase))
            ords[self.n_main:] = (self._ordinal_base(gen - 1) + M + np.arange(N_EVAL)) if with_prev_eval else 0
            ro.reset_from_ordinals(ords)
        ro.run(self.n_cycles)

    def eval_only(self, gen):
        """flush: the evaluation games of generation `gen` alone (main games disabled) -> their mean triple"""
        ro, M = self.ro, 3 * self.pop * self.hof
        ro.set_limits(eval_gate_limits(self.plan.n_games, self.n_main, 0, self.T_eval, 1))
        if self.env_mode == "device":
            ro.reset(0, self.n_main, 0)
            ro.reset(self.n_main, N_EVAL, self._ordinal_base(gen) + M)
        else:
            ords = np.zeros(self.plan.n_games, dtype=np.int64)
            ords[self.n_main:] = self._ordinal_base(gen) + M + np.arange(N_EVAL)
            ro.reset_from_ordinals(ords)
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


class CoGATail:
    """The generation tail of the fully connected Co-GA engines after the rollout: selection, promotion (elites, Hall of Fame,
    best), children with their stale-agent distances - each launch sequence written once, in its fused form (one launch for
    the three roles: E <= 8, hof <= 16, pop <= 4096) and its launch-per-step form.  A class names its promotion, child and
    distance-reduction entry points.  Needs pop, hof, E, philox_seed, slab / base / stride (SlabIO._ptr), dist, div, fitness,
    order, best_dist, dist_partial, pblocks, parent_idx and, for the launch-per-step forms, iota and hof_shift_idx."""
    _promote_entry = "coevo_ga_promote"
    _perturb_dist_entry = "coevo_fc_perturb_dist"
    _finalize_entry = "coevo_fc_distance_finalize"

    def _select_roles(self, rewards_ptr_of, game_first_of, games_per_individual):
        roles = (L.GaSelectRole * 3)()
        for ri, r in enumerate(ROLES):
            roles[ri] = L.GaSelectRole(L._p(self.dist[r]), rewards_ptr_of(ri), L._p(self.div[r]), L._p(self.fitness[r]),
                                       L._p(self.order[r]), L._p(self.best_dist[r]), game_first_of(ri), RET_SLOT[r])
        L.call("coevo_ga_select", roles, 3, self.pop, games_per_individual, self.hof)

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
        if rebuild is not None:
            L.call("coevo_ga_promote_rebuild", roles, 3, self.E, self.hof, L._p(self.sigma32_prev), self.philox_seed, *rebuild)
        elif tick:
            L.call("coevo_ga_promote_tick", roles, 3, self.E, self.hof, L._p(self.gen_dev))
        else:
            L.call(self._promote_entry, roles, 3, self.E, self.hof)

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


class CoESSchedule:
    """The Co-ES training and evaluation rollouts of one generation (game ordinal 3j + role, then the evaluation games).
    Needs pop, lo, n_main, first_ordinal, T_train, T_eval, env_mode, plan, ro, eval_ro."""

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
