"""Baseline gauntlet: a generation's champions against seats that never change, every game in ONE launch.

Fitness in a coevolutionary run is relative; the absolute number is the score against opponents that never change.
``BaselineCrossPlay`` (baselines.py) plays such tables after training with the launches of a training rollout - four per
env-cycle - which is the right form for thousands of games and too slow for the few dozen a trainer wants every generation.
``Gauntlet`` plays a list of matches in coevo_mpe_gauntlet (csrc/gauntlet.hip, include/coevo_gauntlet.h): one workgroup per
game, all its env-cycles in a loop, the same arithmetic and the same words as the per-cycle route.

``Gauntlet``        a list of matches (agent_0 seat, agent_1 seat, adversary seat), E episodes each, game m E + e under reset
                    ordinal first_ordinal + e (``BaselineCrossPlay``'s rule: every match meets the same episodes)
``Champion(role)``  a seat whose weights are set later (``set_champion``): the trainer's newest Hall-of-Fame member
``GauntletSpec``    what a trainer is asked to score every generation (``args.coevo_gauntlet``, GATrainer)

What cannot be served is refused with ValueError before the library is loaded.  float32 nets, one rank, env on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L
from .baselines import MLP_NACT, ROLE_SLOT, MLPBaseline, ScriptedBaseline, mlp_stride
from .crossplay import MAX_GAMES, _check_first_ordinal, _flat, fc_params
from .mpe.simple_adversary import ENV_SEED, INTEGRATE_POS_FIRST
from .population import ROLE_D, ROLES
from .rollout import effective_steps

GT_FC, GT_MLP, GAME_WORDS = L.K_GT["COEVO_GT_FC"], L.K_GT["COEVO_GT_MLP"], L.K_GT["COEVO_GT_GAME_WORDS"]
TRIO = ("agent_0", "agent_1", "adversary_0")   # the order of a match and of a reward triple (play_game's return order)
assert TRIO == tuple(ROLES)


def fc_stride(D):
    """coevo_fc_slab_stride(D) without the library: the parameters rounded up to a multiple of 64 floats"""
    return (fc_params(D) + 63) // 64 * 64


class Champion:
    """the seat of `role` whose weights are set later with ``Gauntlet.set_champion(role, ...)``; every ``Champion(role)`` of a
    match list is the same net"""

    def __init__(self, role):
        if role not in ROLES:
            raise ValueError(f"Champion: role {role!r} (one of {ROLES})")
        self.role = role

    def __repr__(self):
        return f"Champion({self.role!r})"


class GauntletResult:
    """rewards [M][E][3] float64 per game in play_game's return order (agent_0, agent_1, adversary_0), mean [M][3]: per match
    (((+0.0 + rewards[m][0]) + rewards[m][1]) + ...) / E, reduced on the device (coevo_crossplay_reduce's payoff)"""

    def __init__(self, rewards, mean):
        self.rewards, self.mean = rewards, mean
        self.n_games = int(rewards.shape[0] * rewards.shape[1])


class GauntletPlan:
    """The host half of a ``Gauntlet``: the refusals, where every net lies and the game table - no device, no library.
    seats[m][role] = ("script", baseline) / ("mlp", index) / ("fc", index) / ("champion", role); fc_off / mlp_off: float
    offsets into the two slabs; words [M E][COEVO_GT_GAME_WORDS] int32 (include/coevo_gauntlet.h); episode [M E] int64."""

    def __init__(self, matches, episodes=10, what="Gauntlet"):
        if int(episodes) < 1:
            raise ValueError(f"{what}: episodes {episodes} (at least 1)")
        if matches is None or len(matches) == 0:
            raise ValueError(f"{what}: no match")
        from .fcnetwork import FCNetworkHalf
        self.episodes = E = int(episodes)
        self.seats, self.fc_flats, self.fc_role, self.fc_off, self.mlps, self.mlp_off = [], [], [], [], [], []
        self.champion_off, slab, mlp_floats = {}, 0, 0
        for m, trio in enumerate(matches):
            if len(trio) != 3:
                raise ValueError(f"{what}: match {m} is not a trio (agent_0 seat, agent_1 seat, adversary seat)")
            seats = {}
            for role, x in zip(TRIO, trio):
                here = f"{what}: match {m}, role {role}"
                if isinstance(x, Champion):
                    if x.role != role:
                        raise ValueError(f"{here}: the seat is {x!r}")
                    if role not in self.champion_off:
                        self.champion_off[role] = slab
                        slab += fc_stride(ROLE_D[role])
                    seats[role] = ("champion", role)
                elif isinstance(x, ScriptedBaseline):
                    x.check(here, MLP_NACT)
                    seats[role] = ("script", x)
                elif isinstance(x, MLPBaseline):
                    if x.D != ROLE_D[role]:
                        raise ValueError(f"{here}: a policy net of width {x.D}, not {ROLE_D[role]}")
                    seats[role] = ("mlp", len(self.mlps))
                    self.mlps.append(x)
                    self.mlp_off.append(mlp_floats)
                    mlp_floats += mlp_stride(x.D)
                else:
                    if isinstance(getattr(x, "model", x), FCNetworkHalf):
                        raise ValueError(f"{here}: a float16 net (float32 evolved nets only)")
                    f = _flat(x)
                    if f.size != fc_params(ROLE_D[role]):
                        raise ValueError(f"{here}: a net of {f.size} parameters, not {fc_params(ROLE_D[role])}")
                    seats[role] = ("fc", len(self.fc_flats))
                    self.fc_flats.append(f)
                    self.fc_role.append(role)
                    self.fc_off.append(slab)
                    slab += fc_stride(ROLE_D[role])
            self.seats.append(seats)
        self.n_matches = M = len(self.seats)
        self.n_games = M * E
        if self.n_games > MAX_GAMES:
            raise ValueError(f"{what}: {self.n_games} games (at most {MAX_GAMES})")
        if max(slab, mlp_floats) >= 1 << 31:
            raise ValueError(f"{what}: the nets of {M} matches leave the 32-bit offsets of a game word")
        self.slab_floats, self.mlp_floats = slab, mlp_floats
        match_words = np.zeros((M, GAME_WORDS), dtype=np.int64)
        for m, seats in enumerate(self.seats):
            for role in ROLES:
                match_words[m, 4 * ROLE_SLOT[role]:4 * ROLE_SLOT[role] + 4] = self.seat_words(seats[role])
        self.words = np.repeat(match_words, E, axis=0).astype(np.uint32).view(np.int32)
        self.episode = np.tile(np.arange(E, dtype=np.int64), M)

    def net_off(self, seat):
        kind, j = seat
        return self.champion_off[j] if kind == "champion" else self.fc_off[j] if kind == "fc" else self.mlp_off[j]

    def seat_words(self, seat):
        """{kind, arg, seed low word, seed high word} of one seat"""
        kind, x = seat
        if kind == "script":
            return (x.kind, x.arg, x.seed & 0xFFFFFFFF, x.seed >> 32)
        return (GT_MLP if kind == "mlp" else GT_FC, self.net_off(seat), 0, 0)

    def describe(self):
        """one name per match: "agent_0 seat + agent_1 seat vs adversary seat\""""
        def name(seat):
            kind, x = seat
            return repr(x) if kind == "script" else f"Champion({x})" if kind == "champion" else f"{kind}{x}"
        return [f"{name(s['agent_0'])} + {name(s['agent_1'])} vs {name(s['adversary_0'])}" for s in self.seats]


def _device_ptr(src):
    """a device address given as an int or as a device tensor, else None"""
    if torch.is_tensor(src):
        if not src.is_cuda:
            return None
        assert src.is_contiguous() and src.dtype == torch.float32, "a float32 net in the fc slab layout"
        return src.data_ptr()
    if isinstance(src, (int, np.integer)) and not isinstance(src, bool):
        return int(src)
    return None


class Gauntlet:
    """``matches``: a list of trios (agent_0 seat, agent_1 seat, adversary seat); a seat is what ``BaselineCrossPlay`` accepts -
    an FCNetwork, a flat float32 array, an Agent, a scripted baseline, an ``MLPBaseline`` of the role's width - or
    ``Champion(role)``.  ``run(first_ordinal)`` plays game m E + e from reset ordinal first_ordinal + e for
    T = effective_steps(limit, max_cycles) agent-steps with four launches on the current stream - coevo_mpe_reset_episodes,
    coevo_mpe_gauntlet, coevo_mpe_rewards, coevo_crossplay_reduce - and returns a ``GauntletResult`` with the words
    ``BaselineCrossPlay`` gives for the same games; ``enqueue`` does the same without reading back and ``result()`` reads what
    the last enqueue left.  A net whose forward faults raises play_game's ValueError."""

    def __init__(self, matches, episodes=10, limit=None, max_cycles=25, env_seed=ENV_SEED, device="cuda"):
        self.plan = plan = GauntletPlan(matches, episodes)
        self.episodes, self.device, self.n_games, self.n_matches = plan.episodes, device, plan.n_games, plan.n_matches
        self.T = effective_steps(limit, max_cycles)
        self._champion_set = dict.fromkeys(plan.champion_off, False)
        n, f64 = self.n_games, dict(dtype=torch.float64, device=device)
        self.slab = torch.zeros(max(plan.slab_floats, 4), dtype=torch.float32, device=device)
        for f, role, off in zip(plan.fc_flats, plan.fc_role, plan.fc_off):
            self._pack(f, role, off)
        host = np.zeros(max(plan.mlp_floats, 4), dtype=np.float32)
        for m, o in zip(plan.mlps, plan.mlp_off):
            host[o:o + m.flat.size] = m.flat
        self.mlp_slab = torch.from_numpy(host).to(device)
        self.games = torch.from_numpy(plan.words).to(device)
        self.game_episode = torch.from_numpy(plan.episode).to(device)   # int64: a game's ordinal is first_ordinal + its episode
        self.state = torch.zeros(L.MPE_STATE_DOUBLES, n, **f64)
        self.limits = torch.full((n,), self.T, dtype=torch.int32, device=device)
        self.obs = torch.zeros(3 * n, L.OBS_STRIDE, dtype=torch.float32, device=device)
        self.actions = torch.zeros(3 * n, dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.rewards = torch.zeros(n, 3, **f64)
        self.mean = torch.zeros(self.n_matches, 3, **f64)
        self.iota = torch.zeros(1, dtype=torch.int32, device=device)
        self.rng = L.PCG64State.from_seed(env_seed)
        self.pos_first = 1 if INTEGRATE_POS_FIRST else 0
        self._done = None
        torch.cuda.current_stream().synchronize()

    # ---- weights -----------------------------------------------------------------------------------------------------
    def _ptr(self, off):
        return self.slab.data_ptr() + 4 * off

    def _pack(self, flat, role, off):
        flat = torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float32)[None]).to(self.device)
        L.call("coevo_fc_pack", L._p(flat), self._ptr(off), 1, ROLE_D[role])

    def _put_fc(self, what, role, off, src, stream):
        """a flat parameter array (packed into the slab) or a device address of a net in the fc slab layout (copied slab to
        slab by coevo_fc_gather: no host round trip)"""
        with torch.cuda.stream(stream):
            ptr = _device_ptr(src)
            if ptr is not None:
                L.call("coevo_fc_gather", ptr, L._p(self.iota), self._ptr(off), 0, 1, ROLE_D[role])
                return
            flat = _flat(src)
            if flat.size != fc_params(ROLE_D[role]):
                raise ValueError(f"{what}: {flat.size} parameters, not {fc_params(ROLE_D[role])}")
            self._pack(flat, role, off)

    def set_champion(self, role, src, stream=None):
        """the weights of every ``Champion(role)`` seat from now on: a flat float32 array (an FCNetwork, an Agent), or a device
        address / float32 device tensor of a net in the fc slab layout - copied slab to slab on `stream` (default: the current)"""
        if role not in self._champion_set:
            raise ValueError(f"Gauntlet.set_champion: no Champion({role!r}) seat in the matches")
        self._put_fc("Gauntlet.set_champion", role, self.plan.champion_off[role], src, stream)
        self._champion_set[role] = True

    def upload(self, match, role, flat, stream=None):
        """replaces the evolved net or policy net in seat `role` of match `match`; the next run plays it.  An evolved net may be
        given as a device address like ``set_champion``'s."""
        if role not in ROLES:
            raise ValueError(f"Gauntlet.upload: role {role!r} (one of {ROLES})")
        if not 0 <= int(match) < self.n_matches:
            raise ValueError(f"Gauntlet.upload: match {match} (0 .. {self.n_matches - 1})")
        kind, j = seat = self.plan.seats[int(match)][role]
        if kind == "script":
            raise ValueError(f"Gauntlet.upload: seat {role} of match {match} is scripted: it has no weights")
        if kind == "champion":
            raise ValueError(f"Gauntlet.upload: seat {role} of match {match} is Champion({role!r}): use set_champion")
        if kind == "mlp":
            m = flat if isinstance(flat, MLPBaseline) else MLPBaseline(flat, ROLE_D[role])
            if m.D != ROLE_D[role]:
                raise ValueError(f"Gauntlet.upload: a policy net of width {m.D}, not {ROLE_D[role]}")
            off = self.plan.mlp_off[j]
            with torch.cuda.stream(stream):
                self.mlp_slab[off:off + m.flat.size].copy_(torch.from_numpy(m.flat))
            return
        self._put_fc("Gauntlet.upload", role, self.plan.net_off(seat), flat, stream)

    # ---- games -------------------------------------------------------------------------------------------------------
    def enqueue(self, first_ordinal, stream=None):
        """the four launches of a run on `stream` (default: the current stream); nothing is read back"""
        _check_first_ordinal("Gauntlet", first_ordinal, lambda: self.episodes, 64)
        for role, is_set in self._champion_set.items():
            if not is_set:
                raise ValueError(f"Gauntlet: Champion({role!r}) has no weights yet (set_champion)")
        n = self.n_games
        with torch.cuda.stream(stream):
            self.status.zero_()
            L.call("coevo_mpe_reset_episodes", L._p(self.state), n, 0, n, self.rng, int(first_ordinal), self.episodes)
            L.call("coevo_mpe_gauntlet", L._p(self.slab), self.slab.numel(), L._p(self.mlp_slab), self.mlp_slab.numel(),
                   L._p(self.games), n, L._p(self.game_episode), int(first_ordinal), L._p(self.state), L._p(self.limits), 0,
                   (self.T + 2) // 3, self.pos_first, L._p(self.obs), L._p(self.actions), L._p(self.status))
            L.call("coevo_mpe_rewards", L._p(self.state), n, L._p(self.rewards))
            L.call("coevo_crossplay_reduce", L._p(self.rewards), self.n_matches, 1, 1, self.episodes, L._p(self.mean), None,
                   None, None)
            self._done = torch.cuda.Event()
            self._done.record()

    def result(self):
        """what the last enqueue left (waits for it); a faulted forward raises play_game's ValueError"""
        if self._done is None:
            raise ValueError("Gauntlet.result: nothing was enqueued")
        self._done.synchronize()
        L.raise_on_status(self.status)
        return GauntletResult(self.rewards.cpu().numpy().reshape(self.n_matches, self.episodes, 3), self.mean.cpu().numpy())

    def run(self, first_ordinal):
        self.enqueue(first_ordinal)
        return self.result()


# --------------------------------------------------------------------------------------------------------- the trainer's spec
class GauntletSpec:
    """What a Co-GA trainer scores every generation (``args.coevo_gauntlet`` / ``GATrainer(..., gauntlet=...)``):
    ``adversaries``: baselines for the adversary seat, each facing the generation's champion pair (agent_0, agent_1);
    ``agent_pairs``: (agent_0 baseline, agent_1 baseline) pairs, each facing the champion adversary; ``episodes`` games per
    match under the FIXED reset ordinals first_ordinal .. first_ordinal + episodes - 1 - the same episodes every generation, so
    the yardstick does not move.  A dict with these keys is accepted in its place."""

    def __init__(self, adversaries=(), agent_pairs=(), episodes=10, first_ordinal=1):
        self.adversaries, self.agent_pairs = list(adversaries), [tuple(p) for p in agent_pairs]
        self.episodes, self.first_ordinal = int(episodes), int(first_ordinal)
        what = "coevo_gauntlet"
        if not self.adversaries and not self.agent_pairs:
            raise ValueError(f"{what}: no baseline to face (adversaries and agent_pairs are both empty)")
        if any(len(p) != 2 for p in self.agent_pairs):
            raise ValueError(f"{what}: agent_pairs holds (agent_0 baseline, agent_1 baseline) pairs")
        for x in self.adversaries + [b for p in self.agent_pairs for b in p]:
            if not isinstance(x, (ScriptedBaseline, MLPBaseline)):
                raise ValueError(f"{what}: {x!r} is not a baseline (RandomBaseline, PeriodicBaseline, ConstantBaseline, MLPBaseline)")
        _check_first_ordinal(what, self.first_ordinal, lambda: self.episodes, 64)
        self.plan = GauntletPlan(self.matches(), self.episodes, what)   # the remaining refusals, without a device

    @classmethod
    def of(cls, spec):
        if isinstance(spec, cls):
            return spec
        if isinstance(spec, dict):
            unknown = set(spec) - {"adversaries", "agent_pairs", "episodes", "first_ordinal"}
            if unknown:
                raise ValueError(f"coevo_gauntlet: unknown keys {sorted(unknown)}")
            return cls(**spec)
        raise ValueError(f"coevo_gauntlet: a GauntletSpec or a dict, not {type(spec).__name__}")

    def matches(self):
        a0, a1, adv = Champion("agent_0"), Champion("agent_1"), Champion("adversary_0")
        return [(a0, a1, b) for b in self.adversaries] + [(p, q, adv) for p, q in self.agent_pairs]

    def champion_roles(self):
        return tuple(self.plan.champion_off)

    def names(self):
        return self.plan.describe()
