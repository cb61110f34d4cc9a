"""Baseline opponents in cross-play: seats that are not evolved nets.

Fitness in a coevolutionary run is relative; the fixed yardstick is to play every saved member against opponents that never
change.  The reference ships two: the dummy policies of utils/utils_policies.py (``RandomPolicy`` is main.py --test's default
Atari opponent) and three trained PPO policies for simple_adversary_v3 (PPO/model_*.pth, 10/8 -> 64 -> 64 -> 5 ReLU nets
played deterministically by PPO/test_PPO.py).  Here they are seat kinds of a cross-play table:

``RandomBaseline`` ``PeriodicBaseline`` ``ConstantBaseline`` (``AlwaysFire``)   the scripted kinds, ``scripted_action`` below
``MLPBaseline``            a PPO policy net (``from_state_dict``, ``load_ppo_baseline``)
``BaselineCrossPlay``      ``CrossPlay`` whose three lists may mix FCNetworks and baselines of every kind
``DQNBaselineCrossPlay``   ``DQNCrossPlay`` with one side scripted

Departures from the reference, on purpose: ``RandomPolicy`` there draws from Python's unseeded global ``random`` and
``PeriodicPolicy`` keeps its counter from game to game; here the random seat is a counter-based draw keyed by (seed, the game's
reset ordinal, the env slot, the seat's own step count) and the periodic seat restarts with every game - a game is reproducible
from its ordinal alone, and every trio of a table meets the same random opponent in episode e.  The PPO policy is played by the
first maximum of its logits (the project's rule), not ``argmax(softmax(logits))``; PPO training is not built.

What cannot be served is refused with ValueError before the library is loaded.  float32 evolved nets, one rank, env on the
device.  Kernels: csrc/baseline.hip, declared in include/coevo_baseline.h.
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L
from .atari_synthetic import SYNTH_SEED, philox4x32_10
from .crossplay import (MAX_GAMES, CrossPlayResult, _check_first_ordinal, _CrossBase, _CrossSlab, _flat, dqn_params,
                        fc_params)
from .mpe.simple_adversary import ENV_SEED, INTEGRATE_POS_FIRST
from .population import ROLE_D, ROLES, ROLES2, SlabIO
from .rollout import HEAVY_ROWS, LIGHT_ROWS, effective_steps

RANDOM, PERIODIC, CONSTANT = L.K_BL["COEVO_BL_RANDOM"], L.K_BL["COEVO_BL_PERIODIC"], L.K_BL["COEVO_BL_CONSTANT"]
MLP_H, MLP_NACT, MLP_ROW_TILE = L.K_BL["COEVO_MLP_H"], L.K_BL["COEVO_MLP_NACT"], L.K_BL["COEVO_MLP_ROW_TILE"]
ROLE_SLOT = {"adversary_0": 0, "agent_0": 1, "agent_1": 2}   # the env slot of a role (include/coevo.h COEVO_SLOT_*)
_U64 = (1 << 64) - 1


def scripted_action(kind, arg, seed, ordinal, slot, k, n_actions):
    """The action of a scripted seat - the statement the kernel coevo_baseline_actions implements word for word.  `k`: how
    many actions the seat has taken in this game, `ordinal`: the game's reset ordinal, `slot`: the env slot (0 adversary_0,
    1 agent_0, 2 agent_1; the parity in the two-player games)."""
    n_actions = int(n_actions)
    if not 1 <= n_actions <= 32:
        raise ValueError(f"scripted_action: {n_actions} actions (1 .. 32)")
    k = int(k) & 0xFFFFFFFF
    if kind == RANDOM:
        ordinal, seed = int(ordinal) & _U64, int(seed) & _U64
        w = int(philox4x32_10(ordinal & 0xFFFFFFFF, ordinal >> 32, k, int(slot) & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32)[0])
        return (w * n_actions) >> 32
    if kind == PERIODIC:
        if int(arg) < 0:
            raise ValueError(f"scripted_action: periodic start {arg} is negative")
        return (int(arg) + k) % n_actions
    if kind == CONSTANT:
        if not 0 <= int(arg) < n_actions:
            raise ValueError(f"scripted_action: constant action {arg} outside 0 .. {n_actions - 1}")
        return int(arg)
    raise ValueError(f"scripted_action: kind {kind!r}")


class ScriptedBaseline:
    """a seat played by ``scripted_action(kind, arg, seed, ...)``"""
    kind, arg, seed = None, 0, 0

    def action(self, ordinal, slot, k, n_actions):
        return scripted_action(self.kind, self.arg, self.seed, ordinal, slot, k, n_actions)

    def check(self, what, n_actions):
        if self.kind == CONSTANT and not 0 <= self.arg < int(n_actions):
            raise ValueError(f"{what}: constant action {self.arg} outside 0 .. {int(n_actions) - 1}")

    def __repr__(self):
        return f"{type(self).__name__}({self.seed if self.kind == RANDOM else self.arg})"


class RandomBaseline(ScriptedBaseline):
    """utils_policies.RandomPolicy, reproducible: a uniform action per step, keyed by (seed, ordinal, slot, step)"""
    kind = RANDOM

    def __init__(self, seed=0):
        if not 0 <= int(seed) <= _U64:
            raise ValueError(f"RandomBaseline: seed {seed} is not a 64-bit word")
        self.seed = int(seed)


class PeriodicBaseline(ScriptedBaseline):
    """utils_policies.PeriodicPolicy: actions start, start + 1, ... modulo the action count, from `start` again in every game"""
    kind = PERIODIC

    def __init__(self, start=0):
        if not 0 <= int(start) < 1 << 31:
            raise ValueError(f"PeriodicBaseline: start {start} (0 .. 2**31 - 1)")
        self.arg = int(start)


class ConstantBaseline(ScriptedBaseline):
    """utils_policies.AlwaysFirePolicy for any action: the same action at every step"""
    kind = CONSTANT

    def __init__(self, action):
        if not 0 <= int(action) < 32:
            raise ValueError(f"ConstantBaseline: action {action} (0 .. 31, and below the game's action count)")
        self.arg = int(action)


AlwaysFire = ConstantBaseline(1)


def mlp_params(D):
    """coevo_mlp_param_count(D) without the library: fc1, fc2 and the policy head of PPO/PPOagent.py's PPOPolicy"""
    return MLP_H * D + MLP_H + MLP_H * MLP_H + MLP_H + MLP_NACT * MLP_H + MLP_NACT


def mlp_stride(D):
    return (mlp_params(D) + 3) // 4 * 4


_MLP_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "policy_head.weight", "policy_head.bias")


class MLPBaseline:
    """A PPO policy net D -> 64 -> 64 -> 5 (ReLU) as a seat: `flat` in the order fc1.weight [64][D], fc1.bias, fc2.weight
    [64][64], fc2.bias, policy_head.weight [5][64], policy_head.bias - 5189 words for D = 10, 5061 for D = 8; the value head is
    not carried.  Played in fp32: every output one sequential fmaf chain over k ascending from the bias, ReLU v > 0 ? v : +0,
    the action the first maximum of the five logits."""

    def __init__(self, flat, D):
        if int(D) not in (8, 10):
            raise ValueError(f"MLPBaseline: observation width {D} (8 or 10)")
        self.D = int(D)
        self.flat = np.ascontiguousarray(flat, dtype=np.float32).ravel().copy()
        if self.flat.size != mlp_params(self.D):
            raise ValueError(f"MLPBaseline: {self.flat.size} parameters, not {mlp_params(self.D)} for width {self.D}")

    @classmethod
    def from_state_dict(cls, sd):
        """from PPOPolicy.state_dict() (tensors or arrays); value_head.* is dropped"""
        parts = []
        for key in _MLP_KEYS:
            if key not in sd:
                raise ValueError(f"MLPBaseline: the state dict has no {key}")
            v = sd[key]
            parts.append(np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32))
        shapes = [p.shape for p in parts]
        D = shapes[0][1] if len(shapes[0]) == 2 else -1
        if shapes != [(MLP_H, D), (MLP_H,), (MLP_H, MLP_H), (MLP_H,), (MLP_NACT, MLP_H), (MLP_NACT,)]:
            raise ValueError(f"MLPBaseline: not a D -> {MLP_H} -> {MLP_H} -> {MLP_NACT} policy: {shapes}")
        return cls(np.concatenate([p.ravel() for p in parts]), D)


def load_ppo_baseline(path):
    """a checkpoint written by the reference's PPO trainer (torch.save(policy.state_dict(), ...)) -> ``MLPBaseline``"""
    return MLPBaseline.from_state_dict(torch.load(path, map_location="cpu", weights_only=True))


def _is_baseline(x):
    return isinstance(x, (ScriptedBaseline, MLPBaseline))


def _seat_words(game, row, b, slot):
    """[len(game)][COEVO_BL_SEAT_WORDS] int32 of one scripted baseline"""
    w = np.zeros((len(game), L.K_BL["COEVO_BL_SEAT_WORDS"]), dtype=np.int64)
    w[:, 0], w[:, 1], w[:, 2], w[:, 3] = game, row, b.kind, b.arg
    w[:, 4], w[:, 5], w[:, 6] = b.seed & 0xFFFFFFFF, b.seed >> 32, slot
    return w.astype(np.uint32).view(np.int32)


def _dev_words(arr, device, words):
    a = np.ascontiguousarray(arr, dtype=np.int32).reshape(-1, words)
    return torch.from_numpy(a if len(a) else np.zeros((1, words), dtype=np.int32)).to(device)


# ------------------------------------------------------------------------------------------------------- simple_adversary
class BaselineCrossPlay(_CrossBase):
    """``CrossPlay`` whose lists may mix evolved nets (FCNetworks, flat float32 arrays, Agents) with baselines of every kind; an
    ``MLPBaseline`` needs the width of its role.  Same game numbering g = ((a B + b) C + c) E + e, same ordinal rule, same
    reduction and result type.  ``run(first_ordinal)`` enqueues, per env-cycle and on one stream, coevo_mpe_policy_cycle over
    the evolved nets' tasks, coevo_mpe_mlp_policy_cycle, coevo_baseline_actions and coevo_mpe_step; then coevo_mpe_rewards and
    coevo_crossplay_reduce.  ``upload(role, i, flat)`` replaces an evolved net or a policy net between runs."""
    _roles, _D_of = ROLES, ROLE_D

    def __init__(self, agent_0, agent_1, adversary, episodes=10, limit=None, max_cycles=25, precision="float32",
                 env_seed=ENV_SEED, device="cuda"):
        what = "BaselineCrossPlay"
        if precision != "float32":
            raise ValueError(f"{what}: float32 evolved nets only, not precision {precision!r}")
        if int(episodes) < 1:
            raise ValueError(f"{what}: episodes {episodes} (at least 1)")
        from .fcnetwork import FCNetworkHalf
        self._params = {r: fc_params(ROLE_D[r]) for r in ROLES}
        self._entry, fc_flats, mlps = {}, {r: [] for r in ROLES}, []
        for role, seats in (("agent_0", agent_0), ("agent_1", agent_1), ("adversary_0", adversary)):
            if seats is None or len(seats) == 0:
                raise ValueError(f"{what}: no seat for role {role}")
            self._entry[role] = []
            for i, x in enumerate(seats):
                if isinstance(x, ScriptedBaseline):
                    x.check(f"{what}: seat {i} of role {role}", MLP_NACT)
                    self._entry[role].append(("script", x))
                elif isinstance(x, MLPBaseline):
                    if x.D != ROLE_D[role]:
                        raise ValueError(f"{what}: seat {i} of role {role} is a policy net of width {x.D}, not {ROLE_D[role]}")
                    self._entry[role].append(("mlp", len(mlps)))
                    mlps.append(x)
                else:
                    if isinstance(getattr(x, "model", x), FCNetworkHalf):
                        raise ValueError(f"{what}: seat {i} of role {role} is a float16 net (float32 evolved nets only)")
                    f = _flat(x)
                    if f.size != self._params[role]:
                        raise ValueError(f"{what}: net {i} of role {role} has {f.size} parameters, not {self._params[role]}")
                    self._entry[role].append(("fc", len(fc_flats[role])))
                    fc_flats[role].append(f)
        A, B, C = (len(self._entry[r]) for r in ROLES)
        E = int(episodes)
        if A * B * C * E > MAX_GAMES:
            raise ValueError(f"{what}: {A * B * C * E} games (at most {MAX_GAMES})")
        self.episodes, self.precision, self.device = E, precision, device
        self.T = effective_steps(limit, max_cycles)
        self.n_games = n = A * B * C * E
        # ---- the slabs: the evolved nets as CrossPlay keeps them, the policy nets in flat order at 16-byte-aligned offsets
        stride = {r: L.fc_slab_stride(ROLE_D[r]) for r in ROLES}
        self.counts = {r: len(fc_flats[r]) for r in ROLES}
        self.io = _CrossSlab(ROLES, self.counts, stride, self._params, torch.float32, SlabIO._pack_unpack, lambda r: (ROLE_D[r],),
                             device)
        if self.io.slab.numel() == 0:
            self.io.slab = torch.zeros(4, dtype=torch.float32, device=device)
        keep = [self.io.upload(r, "cross", 0, np.stack(fc_flats[r])) for r in ROLES if fc_flats[r]]
        self._mlp_off, off = [], 0
        for m in mlps:
            self._mlp_off.append(off)
            off += mlp_stride(m.D)
        self._mlp_D = [m.D for m in mlps]
        host = np.zeros(max(off, 4), dtype=np.float32)
        for m, o in zip(mlps, self._mlp_off):
            host[o:o + m.flat.size] = m.flat
        self.mlp_slab = torch.from_numpy(host).to(device)
        torch.cuda.current_stream().synchronize()
        del keep
        # ---- the tables: rows of the evolved nets' tasks first (shared-opponent chunks, then per-individual tasks, as
        # RolloutPlan cuts them), then the policy nets' seats, then the scripted seats
        g = np.arange(n, dtype=np.int64)
        index = {"agent_0": g // (B * C * E), "agent_1": (g // (C * E)) % B, "adversary_0": (g // E) % C}
        heavy, light, mlp_tasks, mlp_seats, script_seats = [], [], [], [], []
        row_game, row_slot = [], []
        game_rows = np.zeros((n, 3), dtype=np.int32)
        n_rows = 0

        def take(games, slot):
            nonlocal n_rows
            rows = np.arange(n_rows, n_rows + len(games), dtype=np.int64)
            n_rows += len(games)
            row_game.append(games)
            row_slot.append(np.full(len(games), slot, dtype=np.int64))
            game_rows[games, slot] = rows
            return rows

        fc_sets = [(role, i, np.nonzero(index[role] == i)[0]) for role in ROLES for i, (kind, _) in enumerate(self._entry[role])
                   if kind == "fc"]
        for want_heavy in (True, False):
            for role, i, games in fc_sets:
                if (len(games) > LIGHT_ROWS) != want_heavy:
                    continue
                off = self.io.base[role]["cross"] + self._entry[role][i][1] * stride[role]
                for lo in range(0, len(games), HEAVY_ROWS if want_heavy else LIGHT_ROWS):
                    chunk = games[lo:lo + (HEAVY_ROWS if want_heavy else LIGHT_ROWS)]
                    rows = take(chunk, ROLE_SLOT[role])
                    (heavy if want_heavy else light).append((off, int(rows[0]), len(chunk), ROLE_D[role], 0))
        for role in ROLES:
            for i, (kind, j) in enumerate(self._entry[role]):
                if kind != "mlp":
                    continue
                games = np.nonzero(index[role] == i)[0]
                rows = take(games, ROLE_SLOT[role])
                for lo in range(0, len(games), MLP_ROW_TILE):
                    cnt = min(MLP_ROW_TILE, len(games) - lo)
                    mlp_tasks.append((self._mlp_off[j], sum(len(s) for s in mlp_seats) + lo, cnt, ROLE_D[role]))
                mlp_seats.append(np.stack([games, rows, np.full(len(games), ROLE_SLOT[role]), np.zeros(len(games), dtype=np.int64)],
                                          axis=1))
        for role in ROLES:
            for i, (kind, b) in enumerate(self._entry[role]):
                if kind == "script":
                    games = np.nonzero(index[role] == i)[0]
                    script_seats.append(_seat_words(games, take(games, ROLE_SLOT[role]), b, ROLE_SLOT[role]))
        assert n_rows == 3 * n
        self.n_rows = n_rows
        self.heavy_np = np.array(heavy, dtype=L.TASK_DTYPE) if heavy else np.zeros(0, L.TASK_DTYPE)
        self.light_np = np.array(light, dtype=L.TASK_DTYPE) if light else np.zeros(0, L.TASK_DTYPE)
        self._fc_tables = [(L.tasks_to_device(t, device), len(t), int(t["n_rows"].max()))
                           for t in (self.heavy_np, self.light_np) if len(t)]
        self.n_mlp_tasks = len(mlp_tasks)
        self.n_mlp_seats = sum(len(s) for s in mlp_seats)
        self.mlp_tasks = _dev_words(mlp_tasks, device, L.K_BL["COEVO_MLP_TASK_WORDS"])
        self.mlp_seats = _dev_words(np.concatenate(mlp_seats) if mlp_seats else [], device, L.K_BL["COEVO_MLP_SEAT_WORDS"])
        self.n_script = sum(len(s) for s in script_seats)
        self.script_seats = _dev_words(np.concatenate(script_seats) if script_seats else [], device,
                                       L.K_BL["COEVO_BL_SEAT_WORDS"])
        dev32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)   # noqa: E731
        self.row_game, self.row_slot = dev32(np.concatenate(row_game)), dev32(np.concatenate(row_slot))
        self.game_rows = dev32(game_rows.reshape(-1))
        self.game_episode = torch.from_numpy(g % E).to(device)   # int64: a game's ordinal is first_ordinal + its episode
        self.state = torch.zeros(L.MPE_STATE_DOUBLES, n, dtype=torch.float64, device=device)
        self.actions = torch.zeros(n_rows, dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.limits = torch.full((n,), self.T, dtype=torch.int32, device=device)
        self.rewards = torch.zeros(n, 3, dtype=torch.float64, device=device)
        self.rng = L.PCG64State.from_seed(env_seed)
        self.pos_first = 1 if INTEGRATE_POS_FIRST else 0
        self._reduce_buffers((A, B, C))

    def upload(self, role, i, flat):
        """replaces evolved net or policy net i of `role` (a scripted seat has no weights); the next run() plays it"""
        name = type(self).__name__
        if role not in ROLES:
            raise ValueError(f"{name}: role {role!r} (one of {ROLES})")
        if not 0 <= int(i) < len(self._entry[role]):
            raise ValueError(f"{name}: seat {i} of role {role} (0 .. {len(self._entry[role]) - 1})")
        kind, j = self._entry[role][int(i)]
        if kind == "script":
            raise ValueError(f"{name}: seat {i} of role {role} is scripted: it has no weights")
        if kind == "mlp":
            m = flat if isinstance(flat, MLPBaseline) else MLPBaseline(flat, self._mlp_D[j])
            if m.D != self._mlp_D[j]:
                raise ValueError(f"{name}: a policy net of width {m.D}, not {self._mlp_D[j]}")
            self.mlp_slab[self._mlp_off[j]:self._mlp_off[j] + m.flat.size].copy_(torch.from_numpy(m.flat))
            return
        flat = _flat(flat)
        if flat.size != self._params[role]:
            raise ValueError(f"{name}: {flat.size} parameters, not {self._params[role]}")
        keep = self.io.upload(role, "cross", j, flat[None])
        torch.cuda.current_stream().synchronize()
        del keep

    def enqueue_cycle(self, c, first_ordinal):
        """the launches of env-cycle c on the current stream"""
        n = self.n_games
        for tasks, count, max_rows in self._fc_tables:
            L.call("coevo_mpe_policy_cycle", L._p(self.io.slab), L._p(tasks), count, max_rows, L._p(self.state), n,
                   L._p(self.row_game), L._p(self.row_slot), L._p(self.actions), L._p(self.status))
        if self.n_mlp_tasks:
            L.call("coevo_mpe_mlp_policy_cycle", L._p(self.mlp_slab), self.mlp_slab.numel(), L._p(self.mlp_tasks),
                   self.n_mlp_tasks, L._p(self.mlp_seats), self.n_mlp_seats, L._p(self.state), n, L._p(self.actions),
                   self.n_rows, None, L._p(self.status))
        if self.n_script:
            L.call("coevo_baseline_actions", L._p(self.script_seats), self.n_script, L._p(self.game_episode),
                   int(first_ordinal), n, c, MLP_NACT, L._p(self.actions), self.n_rows)
        L.call("coevo_mpe_step", L._p(self.state), n, L._p(self.game_rows), L._p(self.actions), c, L._p(self.limits),
               self.pos_first)

    def run(self, first_ordinal):
        _check_first_ordinal(type(self).__name__, first_ordinal, lambda: self.episodes, 64)
        n = self.n_games
        self.status.zero_()
        L.call("coevo_mpe_reset_episodes", L._p(self.state), n, 0, n, self.rng, int(first_ordinal), self.episodes)
        for c in range((self.T + 2) // 3):
            self.enqueue_cycle(c, first_ordinal)
        L.call("coevo_mpe_rewards", L._p(self.state), n, L._p(self.rewards))
        L.raise_on_status(self.status)
        self._reduce(self.rewards)
        A, B, C = self.dims
        marg = {r: self.marg[k].cpu().numpy() for k, r in enumerate(ROLES)}
        return CrossPlayResult(self.payoff.cpu().numpy().reshape(A, B, C, 3), marg,
                               self.rewards.cpu().numpy().reshape(A, B, C, self.episodes, 3))


# ------------------------------------------------------------------------------------------------------ synthetic Atari
def one_side_tasks(side_nets, net_off):
    """the DeepQN task table of games in which ONE parity is played by nets - game g's net is ``side_nets[g]``, an id into
    net_off - with the rows grouped by net into tasks of <= COEVO_DQN_MAX_ROWS frames -> (tasks [DQN_TASK_DTYPE], the row of
    every game [n] int32)"""
    by_net = {}
    for g, net in enumerate(side_nets):
        by_net.setdefault(int(net), []).append(g)
    tasks, row_of_game, row = [], np.zeros(len(side_nets), dtype=np.int32), 0
    for net, games in by_net.items():
        for i in range(0, len(games), L.DQN_MAX_ROWS):
            chunk = games[i:i + L.DQN_MAX_ROWS]
            tasks.append((int(net_off[net]), row, len(chunk)))
            row_of_game[chunk] = np.arange(row, row + len(chunk))
            row += len(chunk)
    return np.array(tasks, dtype=L.DQN_TASK_DTYPE), row_of_game


class BaselineSynthRollout:
    """``SynthRollout`` (dqn_population.py) for games in which one parity is scripted: game g seats net ``side_nets[g]`` (a net
    id into net_off) on parity `net_parity` and scripted baseline ``seats`` on the other.  On the scripted parity the conv
    stack + fc1 launch is skipped and coevo_dqn_out_synth_step is replaced by coevo_baseline_actions into that parity's action
    row followed by plain coevo_synth_step (which renders no frame for a scripted actor).  One cohort, eager enqueue."""

    def __init__(self, side_nets, net_off, net_parity, script_seats, ordinal0, C, n_actions, slab, env_seed, device="cuda",
                 fc1_tiled=False):
        from .dqn_population import FRAME
        self.n_games = n = len(side_nets)
        self.C, self.n_actions, self.slab, self.env_seed, self.device = C, n_actions, slab, int(env_seed), device
        self.Cw = C | (L.DQN_FC1_TILED if fc1_tiled else 0)
        self.net_parity = int(net_parity)
        self.ordinal0 = torch.from_numpy(np.asarray(ordinal0, dtype=np.int64)).to(device)
        self.gstate = torch.zeros(n, 4, dtype=torch.int32, device=device)
        self.acc = torch.zeros(n, 3, dtype=torch.float64, device=device)
        self.limit = torch.zeros(n, dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.tasks_np, row_of_game = one_side_tasks(side_nets, net_off)
        self.tasks, self.n_tasks = L.tasks_to_device(self.tasks_np, device), len(self.tasks_np)
        self.max_rows = int(self.tasks_np["n_rows"].max())
        # the net parity's rows are its tasks' rows; the scripted parity's action row is indexed by game
        identity = np.arange(n, dtype=np.int32)
        self.rows = [torch.from_numpy(row_of_game if p == self.net_parity else identity).to(device) for p in range(2)]
        self.seats, self.n_seats = _dev_words(script_seats, device, L.K_BL["COEVO_BL_SEAT_WORDS"]), len(script_seats)
        self.frames = torch.zeros(n * FRAME * C, dtype=torch.uint8, device=device)
        self.actions = torch.zeros(2, n, dtype=torch.int32, device=device)
        self.ws = torch.zeros(int(L.load().coevo_dqn_workspace_bytes(n)) // 4, dtype=torch.float32, device=device)

    def set_limits(self, limits):
        self.limit.copy_(torch.from_numpy(np.asarray(limits, dtype=np.int32)))

    def enqueue(self, T, gen_dev=None):
        """T agent-steps of every game + the closing bookkeeping call, on the current stream"""
        assert gen_dev is None
        lib, stream, n = L.load(), L._stream(), self.n_games
        gs, ac, o0, lim = L._p(self.gstate), L._p(self.acc), L._p(self.ordinal0), L._p(self.limit)
        for t in range(T + 1):
            p, q = t & 1, (t - 1) & 1
            net_next = t < T and p == self.net_parity   # a net acts at step t: it needs the frame of step t
            row_cur, frames = (L._p(self.rows[p]), L._p(self.frames)) if net_next else (None, None)
            if t == 0:
                L._check(lib.coevo_synth_step(gs, ac, n, o0, None, 0, t, lim, None, None, row_cur, frames, self.C,
                                              self.n_actions, self.env_seed, stream), "coevo_synth_step")
            elif q == self.net_parity:   # the output layer of step t-1 rides in the env-step launch
                L._check(lib.coevo_dqn_out_synth_step(gs, ac, n, o0, None, 0, t, lim, L._p(self.rows[q]),
                                                      self.actions[q].data_ptr(), row_cur, frames, self.C, self.n_actions,
                                                      self.env_seed, L._p(self.slab), L._p(self.tasks), self.n_tasks, n,
                                                      L._p(self.ws), L._p(self.status), stream), "coevo_dqn_out_synth_step")
            else:
                L._check(lib.coevo_baseline_actions(L._p(self.seats), self.n_seats, o0, 0, n, (t - 1 - q) // 2, self.n_actions,
                                                    self.actions[q].data_ptr(), n, stream), "coevo_baseline_actions")
                L._check(lib.coevo_synth_step(gs, ac, n, o0, None, 0, t, lim, L._p(self.rows[q]), self.actions[q].data_ptr(),
                                              row_cur, frames, self.C, self.n_actions, self.env_seed, stream), "coevo_synth_step")
            if net_next:
                L._check(lib.coevo_dqn_forward_hidden_timed(L._p(self.slab), L._p(self.tasks), self.n_tasks, self.max_rows, n,
                                                            self.Cw, self.n_actions, L._p(self.frames), L._p(self.ws), None, 0,
                                                            stream), "coevo_dqn_forward_hidden_timed")


class DQNBaselineCrossPlay(_CrossBase):
    """``DQNCrossPlay`` with one side scripted: one of `first` / `second` holds DeepQN nets (flat arrays in ``DeepQN.flat()``
    order, nets or Agents), the other scripted baselines (``RandomBaseline``, ``PeriodicBaseline``, ``ConstantBaseline``).  A
    list holds one kind: nets and baselines are not mixed inside it, both lists scripted leaves nothing to evaluate, and an
    ``MLPBaseline`` (a simple_adversary policy) is refused.  Game (a B + b) E + e under reset ordinal first_ordinal + e,
    ``limit`` agent-steps each; a scripted seat's step count k at agent-step t of parity p is (t - p) / 2.  float32 only."""
    _roles, _D_of = ROLES2, None

    def __init__(self, first, second, C, n_actions, episodes=10, limit=None, precision="float32", env_seed=SYNTH_SEED,
                 fc1_layout="streamed", device="cuda"):
        what = "DQNBaselineCrossPlay"
        if precision != "float32":
            raise ValueError(f"{what}: float32 only, not precision {precision!r}")
        if limit is None:
            raise ValueError("the synthetic Atari env never terminates: a step limit is required")
        if int(limit) < 0:
            raise ValueError(f"{what}: negative step limit {limit}")
        if fc1_layout not in ("streamed", "tiled"):
            raise ValueError(f'{what}: fc1_layout is "streamed" or "tiled", not {fc1_layout!r}')
        if not (1 <= int(C) <= 6 and 1 <= int(n_actions) <= 32):
            raise ValueError(f"{what}: {C} channels / {n_actions} actions is not a DeepQN shape")
        if int(episodes) < 1:
            raise ValueError(f"{what}: episodes {episodes} (at least 1)")
        from .deepqn import DeepQNHalf
        self.C, self.n_actions, E = int(C), int(n_actions), int(episodes)
        P = dqn_params(self.C, self.n_actions)
        self._params = dict.fromkeys(ROLES2, P)
        lists, scripted = {"first_0": first, "second_0": second}, {}
        for role, seats in lists.items():
            if seats is None or len(seats) == 0:
                raise ValueError(f"{what}: no seat for role {role}")
            if any(isinstance(x, MLPBaseline) for x in seats):
                raise ValueError(f"{what}: an MLPBaseline is a simple_adversary policy, not an Atari seat")
            kinds = {isinstance(x, ScriptedBaseline) for x in seats}
            if len(kinds) != 1:
                raise ValueError(f"{what}: role {role} mixes nets and scripted baselines (a list holds one kind)")
            scripted[role] = kinds.pop()
        if all(scripted.values()):
            raise ValueError(f"{what}: both sides are scripted: no net to evaluate (use DQNCrossPlay for nets on both sides)")
        if not any(scripted.values()):
            raise ValueError(f"{what}: no scripted side (use DQNCrossPlay for nets on both sides)")
        net_role = next(r for r in ROLES2 if not scripted[r])
        script_role = next(r for r in ROLES2 if scripted[r])
        for i, b in enumerate(lists[script_role]):
            b.check(f"{what}: seat {i} of role {script_role}", self.n_actions)
        flats = []
        for i, x in enumerate(lists[net_role]):
            if isinstance(getattr(x, "model", x), DeepQNHalf):
                raise ValueError(f"{what}: net {i} of role {net_role} is a float16 net (float32 only)")
            f = _flat(x)
            if f.size != P:
                raise ValueError(f"{what}: net {i} of role {net_role} has {f.size} parameters, not {P}")
            flats.append(f)
        A, B = len(first), len(second)
        if A * B * E > MAX_GAMES:
            raise ValueError(f"{what}: {A * B * E} games (at most {MAX_GAMES})")
        self.episodes, self.precision, self.device, self.T = E, precision, device, int(limit)
        self.net_role, self.script_role = net_role, script_role
        tiled = fc1_layout == "tiled"
        stride = int(L.load().coevo_dqn_slab_stride(self.C, self.n_actions))
        if stride <= 0:
            raise ValueError(f"{what}: {C} channels / {n_actions} actions is not a DeepQN shape")
        net_args = self.C | (L.DQN_FC1_TILED if tiled else 0)
        self.counts = {net_role: len(flats), script_role: 0}
        self.io = _CrossSlab(ROLES2, self.counts, dict.fromkeys(ROLES2, stride), self._params, torch.float32,
                             ("coevo_dqn_pack", "coevo_dqn_unpack"), lambda r: (net_args, self.n_actions), device)
        keep = self.io.upload(net_role, "cross", 0, np.stack(flats))
        torch.cuda.current_stream().synchronize()
        del keep
        g = np.arange(A * B * E, dtype=np.int64)
        index = {"first_0": g // (B * E), "second_0": (g // E) % B}
        self._episode = g % E
        net_parity, script_parity = ROLES2.index(net_role), ROLES2.index(script_role)
        net_off = [self.io.base[net_role]["cross"] + i * stride for i in range(len(flats))]
        seats = np.zeros((len(g), L.K_BL["COEVO_BL_SEAT_WORDS"]), dtype=np.int32)
        for i, b in enumerate(lists[script_role]):
            games = np.nonzero(index[script_role] == i)[0]
            seats[games] = _seat_words(games, games, b, script_parity)
        self.ro = BaselineSynthRollout(index[net_role], net_off, net_parity, seats, self._episode, self.C, self.n_actions,
                                       self.io.slab, env_seed, device, fc1_tiled=tiled)
        self._reduce_buffers((A, B, 1))

    def upload(self, role, i, flat):
        if role != self.net_role:
            raise ValueError(f"{type(self).__name__}: role {role!r} has no weights (the nets play {self.net_role})")
        super().upload(role, i, flat)

    def run(self, first_ordinal):
        _check_first_ordinal(type(self).__name__, first_ordinal, lambda: self.episodes, 63)
        ro = self.ro
        ro.status.zero_()
        ro.ordinal0.copy_(torch.from_numpy(int(first_ordinal) + self._episode))
        ro.set_limits(np.full(ro.n_games, self.T, dtype=np.int32))
        ro.enqueue(self.T)
        torch.cuda.synchronize()
        L.raise_on_status(ro.status)
        self._reduce(ro.acc, marg_c=False)
        A, B, _ = self.dims
        marg = {r: self.marg[k].cpu().numpy()[:, :2] for k, r in enumerate(ROLES2)}
        return CrossPlayResult(self.payoff.cpu().numpy().reshape(A, B, 3)[..., :2], marg,
                               ro.acc.cpu().numpy().reshape(A, B, self.episodes, 3)[..., :2])
