"""Cross-play over the paddle duel (``atari_duel``): DeepQN nets against each other and against seats of known skill, a whole
table of games in one rollout, with the points and the endings beside the returns.

The duel is the one DeepQN env here in which play matters, and under the default credit rule "next" the RETURN rewards losing
a point (atari_duel.py): a payoff table of returns alone would mislead, so every result carries the points scored and
whether the game ended.

``TrackerSeat``            the duel's own opponent of known skill (``atari_duel.DuelTracker``) as a device seat
``duel_seat_action``       the one plain-Python statement of what a seat plays; ``duel_tracker_word`` is the tracker's closed form
``DuelSeatRollout`` / ``HalfDuelSeatRollout``   games in which one parity is a net and the other a seat: the seat's whole
                           agent-step happens INSIDE the env-step launch that books the net's (include/coevo_duel_seats.h) -
                           three launches (conv stack, fc1, env) per TWO agent-steps
``DuelCrossPlay``          every first_0 x second_0 of two lists (nets, or seats on one side), ``episodes`` games each
``duel_test_agents`` / ``duel_cross_play_checkpoints``   ``crossplay.test_agents`` / ``cross_play_checkpoints`` for a ``DuelAEC``

What cannot be served is refused with ValueError before the library is loaded.  One rank, frames rendered on the device.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import lib as L
from .atari_duel import CREDITS, PADDLE_H, STATE_WORDS, X0, X1, DuelAEC
from .atari_synthetic import SYNTH_SEED
from .baselines import CONSTANT, PERIODIC, RANDOM, MLPBaseline, ScriptedBaseline, one_side_tasks, scripted_action
from .crossplay import (MAX_GAMES, CrossPlayResult, _check_first_ordinal, _CrossBase, _CrossSlab, _eval_limit, _flat,
                        _precision_of, _take_ordinals, dqn_params)
from .population import ROLES2, NetTable, cross_games2

TRACKER = L.K_DUEL_SEATS["COEVO_DUEL_SEAT_TRACKER"]
SEAT_WORDS = L.K_DUEL_SEATS["COEVO_DUEL_SEAT_WORDS"]
_U64 = (1 << 64) - 1


class TrackerSeat:
    """``atari_duel.DuelTracker`` as a seat: it moves its paddle's centre toward the ball (2 up, 3 down, 0 within 2 pixels),
    read from the newest snapshot.  Tracker against tracker never concedes a point."""
    kind, arg, seed = TRACKER, 0, 0

    def __repr__(self):
        return "TrackerSeat()"


def _is_seat(x):
    return isinstance(x, (ScriptedBaseline, TrackerSeat))


def duel_tracker_word(word, player):
    """the tracker's action for `player` (0 first_0, 1 second_0) from one snapshot word - ``atari_duel.duel_tracker_action`` on
    the frame rendered from it, in closed form (the statement of include/coevo_duel_seats.h)"""
    word, s = int(word) & 0xFFFFFFFF, int(player)
    bx, by = word & 0xFF, (word >> 8) & 0xFF
    p = (word >> 24) & 0xFF if s else (word >> 16) & 0xFF
    X = X1 if s else X0
    hidden = bx <= X <= bx + 1 and by + 1 >= p and by <= p + PADDLE_H - 1   # the ball covers paddle rows in the column read
    top = min(p, by) if hidden else p
    d = 2 * by + 2 - (2 * top + PADDLE_H)
    return 0 if abs(d) <= 4 else (2 if d < 0 else 3)


def duel_seat_action(seat, word15, seed_ordinal, parity, k, n_actions):
    """What `seat` plays: word15 is the newest snapshot (state word 15) when it acts, seed_ordinal the game's reset ordinal
    (with the seat's own seed the key of a random seat's draw), parity the seat's side (0 first_0, 1 second_0), k the number
    of actions it has taken in this game.  The kernel behind coevo_duel_seat_step implements this word for word; an invalid
    seat raises ValueError here and plays 0 (raising COEVO_ST_BAD_TASK) there."""
    if seat.kind == TRACKER:
        return duel_tracker_word(word15, parity)
    if seat.kind in (RANDOM, PERIODIC, CONSTANT):
        return scripted_action(seat.kind, seat.arg, seat.seed, seed_ordinal, parity, k, n_actions)
    raise ValueError(f"duel_seat_action: seat kind {seat.kind!r}")


def seat_words(seat):
    """one row of the seat table: {kind, arg, seed low word, seed high word} as int32"""
    w = np.array([seat.kind, seat.arg, seat.seed & 0xFFFFFFFF, (seat.seed >> 32) & 0xFFFFFFFF], dtype=np.int64)
    return w.astype(np.uint32).view(np.int32)


def _check_seat(what, seat, n_actions):
    if seat.kind not in (RANDOM, PERIODIC, CONSTANT, TRACKER):
        raise ValueError(f"{what}: seat kind {seat.kind!r}")
    if seat.kind == PERIODIC and int(seat.arg) < 0:
        raise ValueError(f"{what}: periodic start {seat.arg} is negative")
    if seat.kind == CONSTANT and not 0 <= int(seat.arg) < int(n_actions):
        raise ValueError(f"{what}: constant action {seat.arg} outside 0 .. {int(n_actions) - 1}")
    if not 0 <= int(seat.seed) <= _U64:
        raise ValueError(f"{what}: seed {seat.seed} is not a 64-bit word")


# ------------------------------------------------------------------------------------------------------------- rollout
class DuelSeatRollout:
    """Duel games in which parity `script_parity` is a scripted seat and the other a float32 DeepQN net: game g seats net
    ``side_nets[g]`` (a net id into net_off) and the seat of row g of ``seat_table`` ([n][4] int32, ``seat_words``).  The task
    table covers the net parity only; one cohort, eager enqueue.

    script_parity 1 (the net is first_0): coevo_duel_step(t = 0) with frame 0, the forward, then the seat launch at t = 1, 3, ...
    (books the net's step t - 1, plays and books the seat's step t, renders the net's frame t + 1) + the forward.
    script_parity 0: seat launches at t = 0, 2, ..., the forward after each that rendered.  The last launch is the closing one
    (t = T) when step T - 1 is the net's.  ``fused_out``: the output layer rides in the seat launch
    (coevo_dqn_out_duel_seat_step after coevo_dqn_forward_hidden_timed); False keeps coevo_dqn_forward_argmax +
    coevo_duel_seat_step - the same words in every buffer."""
    _sym = "coevo_dqn"

    def __init__(self, side_nets, net_off, script_parity, seat_table, ordinal0, C, n_actions, slab, env_seed, device="cuda",
                 fc1_tiled=False, points_to_win=21, credit="next"):
        from .dqn_population import FRAME
        if credit not in CREDITS or int(points_to_win) < 1 or int(C) not in (4, 6) or int(script_parity) not in (0, 1):
            raise ValueError(f"duel seat rollout: credit {credit!r}, points_to_win {points_to_win}, {C} channels or parity "
                             f"{script_parity} out of range")
        self.n_games = n = len(side_nets)
        self.C, self.n_actions, self.slab, self.env_seed, self.device = int(C), int(n_actions), slab, int(env_seed), device
        self.script_parity = int(script_parity)
        self.points_to_win, self.credit = int(points_to_win), credit
        self.flags = L.K_DUEL["COEVO_DUEL_CREDIT_OWN"] if credit == "own" else 0
        self.fc1_tiled, self.fused_out = bool(fc1_tiled), True
        self.ordinal0 = torch.from_numpy(np.asarray(ordinal0, dtype=np.int64)).to(device)
        self.dstate = torch.zeros(n, STATE_WORDS, dtype=torch.int32, device=device)
        self.acc = torch.zeros(n, 3, dtype=torch.float64, device=device)
        self.limit = torch.zeros(n, dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.tasks_np, row_of_game = one_side_tasks(side_nets, net_off)
        self.tasks, self.n_tasks = L.tasks_to_device(self.tasks_np, device), len(self.tasks_np)
        self.max_rows = int(self.tasks_np["n_rows"].max())
        self.rows = torch.from_numpy(row_of_game).to(device)
        seat_table = np.ascontiguousarray(seat_table, dtype=np.int32).reshape(n, SEAT_WORDS)
        self.seats = torch.from_numpy(seat_table).to(device)
        self.frames = torch.zeros(n * FRAME * self.C, dtype=torch.uint8, device=device)
        self.actions = torch.zeros(n, dtype=torch.int32, device=device)          # the nets' actions, by task row
        self.script_actions = torch.zeros(n, dtype=torch.int32, device=device)   # the seats' latest actions, by game
        self.ws = torch.zeros(int(getattr(L.load(), self._sym + "_workspace_bytes")(n)) // 4, dtype=torch.float32, device=device)

    def set_limits(self, limits):
        self.limit.copy_(torch.from_numpy(np.asarray(limits, dtype=np.int32)))

    # the two forward launches of the nets' rows: hidden (the output layer rides in the next seat launch) or to the action
    def _forward(self, lib, stream):
        n = self.n_games
        Cw = self.C | (L.DQN_FC1_TILED if self.fc1_tiled else 0)
        fwd = (L._p(self.slab), L._p(self.tasks), self.n_tasks, self.max_rows, n, Cw, self.n_actions, L._p(self.frames))
        if self.fused_out:
            L._check(lib.coevo_dqn_forward_hidden_timed(*fwd, L._p(self.ws), None, 0, stream), "coevo_dqn_forward_hidden_timed")
        else:
            L._check(lib.coevo_dqn_forward_argmax(*fwd, L._p(self.actions), None, L._p(self.status), L._p(self.ws), stream),
                     "coevo_dqn_forward_argmax")

    def _seat_step(self, lib, t, T, stream):
        render = t + 1 < T
        args = (L._p(self.dstate), L._p(self.acc), self.n_games, L._p(self.ordinal0), None, 0, t, L._p(self.limit),
                L._p(self.seats), self.script_parity, L._p(self.rows) if t else None, L._p(self.actions) if t else None,
                L._p(self.script_actions), L._p(self.rows) if render else None, L._p(self.frames) if render else None, self.C,
                self.n_actions, self.env_seed, self.points_to_win, self.flags)
        if t and self.fused_out:
            entry = self._sym + "_out_duel_seat_step"
            L._check(getattr(lib, entry)(*args, L._p(self.slab), L._p(self.tasks), self.n_tasks, self.n_games, L._p(self.ws),
                                         L._p(self.status), stream), entry)
        else:
            L._check(lib.coevo_duel_seat_step(*args, L._p(self.status), stream), "coevo_duel_seat_step")
        return render

    def steps(self, T):
        """the env launches of a T-step rollout, in order: ("reset", 0) - coevo_duel_step(t = 0), script_parity 1 only - then
        ("seat", t) for t = script_parity, script_parity + 2, ... <= T"""
        return ([("reset", 0)] if self.script_parity else []) + [("seat", t) for t in range(self.script_parity, int(T) + 1, 2)]

    def enqueue_step(self, kind, t, T):
        """one env launch of ``steps(T)`` on the current stream and, when it rendered a frame, the nets' forward"""
        lib, stream, T = L.load(), L._stream(), int(T)
        if kind == "reset":
            render = T > 0
            L._check(lib.coevo_duel_step(L._p(self.dstate), L._p(self.acc), self.n_games, L._p(self.ordinal0), None, 0, 0,
                                         L._p(self.limit), None, None, L._p(self.rows) if render else None,
                                         L._p(self.frames) if render else None, self.C, self.n_actions, self.env_seed,
                                         self.points_to_win, self.flags, stream), "coevo_duel_step")
        else:
            render = self._seat_step(lib, t, T, stream)
        if render:
            self._forward(lib, stream)

    def enqueue(self, T, gen_dev=None):
        """T agent-steps of every game on the current stream, the closing bookkeeping included"""
        assert gen_dev is None
        for kind, t in self.steps(T):
            self.enqueue_step(kind, t, T)


class HalfDuelSeatRollout(DuelSeatRollout):
    """``DuelSeatRollout`` over an fp16 slab (coevo_dqn16_pack's layout, ``net_off`` in 32-bit words):
    coevo_dqn16_out_duel_seat_step after coevo_dqn16_forward_hidden; ``COEVO_DQN16_FUSED_OUT=0``, read at construction, keeps
    coevo_dqn16_forward_argmax + coevo_duel_seat_step, as in ``HalfDuelRollout``.  ``fc1_tiled``: the ``*_tiled`` forward pair."""
    _sym = "coevo_dqn16"

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.fused_out = os.environ.get("COEVO_DQN16_FUSED_OUT", "1") != "0"

    def _forward(self, lib, stream):
        sfx = "_tiled" if self.fc1_tiled else ""
        fwd = (L._p(self.slab), L._p(self.tasks), self.n_tasks, self.max_rows, self.n_games, self.C, self.n_actions,
               L._p(self.frames))
        if self.fused_out:
            entry = "coevo_dqn16_forward_hidden" + sfx
            L._check(getattr(lib, entry)(*fwd, L._p(self.status), L._p(self.ws), stream), entry)
        else:
            entry = "coevo_dqn16_forward_argmax" + sfx
            L._check(getattr(lib, entry)(*fwd, L._p(self.actions), None, L._p(self.status), L._p(self.ws), stream), entry)


# ----------------------------------------------------------------------------------------------------------- cross-play
class DuelCrossPlayResult(CrossPlayResult):
    """``CrossPlayResult`` of the two-player games - payoff [A, B, 2], marginals {role: [n_role, 2]}, rewards [A, B, E, 2]: the
    RETURNS under the table's credit rule - plus what the returns do not say: points [A, B, E, 2] int (the points first_0 and
    second_0 scored, state words 7 and 8), ended [A, B, E] int (state word 11: 0 while the game ran to its step limit, else the
    count of agent-steps booked when a side reached points_to_win) and point_margin [A, B] = the mean over the episodes of
    points[..., 0] - points[..., 1].

    Under credit "next" (the default, play_atari's rule) an actor is credited with the OTHER side's cumulative reward: a HIGHER
    return means MORE points conceded.  Rank nets by ``points`` / ``point_margin``, or build the table with credit "own"."""

    def __init__(self, payoff, marginals, rewards, points, ended):
        super().__init__(payoff, marginals, rewards)
        self.points, self.ended = points, ended
        self.point_margin = (points[..., 0] - points[..., 1]).mean(axis=-1)


class DuelCrossPlay(_CrossBase):
    """Every first_0 x second_0 of two lists over the duel, ``episodes`` games each, in one device rollout.  A list holds DeepQN
    nets (flat arrays in ``DeepQN.flat()`` / ``DeepQNHalf.flat()`` order, nets or Agents) or duel seats (``TrackerSeat``,
    ``RandomBaseline``, ``PeriodicBaseline``, ``ConstantBaseline``) - one kind per list.  Nets on both sides play through
    ``DuelRollout`` / ``HalfDuelRollout``; one scripted side through ``DuelSeatRollout`` / ``HalfDuelSeatRollout``; both sides
    scripted leaves no net to evaluate and is refused.  Game (a B + b) E + e runs under reset ordinal first_ordinal + e for
    ``limit`` agent-steps or until a side has ``points_to_win``; a seat's step count k at agent-step t of parity p is
    (t - p) / 2.  ``run(first_ordinal)`` -> ``DuelCrossPlayResult``; ``upload(role, i, flat)`` replaces a net between runs."""
    _roles, _D_of = ROLES2, None

    def __init__(self, first, second, C, n_actions, episodes=10, limit=None, points_to_win=21, credit="next",
                 precision="float32", env_seed=SYNTH_SEED, fc1_layout="streamed", device="cuda"):
        what = "DuelCrossPlay"
        if precision not in ("float32", "float16"):
            raise ValueError(f"Unsupported precision: {precision}")
        if limit is None:
            raise ValueError(f"{what}: the device route of the duel env plays a fixed number of launches: a step limit is required")
        if int(limit) < 0:
            raise ValueError(f"{what}: negative step limit {limit}")
        if fc1_layout not in ("streamed", "tiled"):
            raise ValueError(f'{what}: fc1_layout is "streamed" or "tiled", not {fc1_layout!r}')
        if int(C) not in (4, 6):
            raise ValueError(f"{what}: the duel env renders 4 or 6 channels, not {C}")
        if not 1 <= int(n_actions) <= 32:
            raise ValueError(f"{what}: {n_actions} actions is not a DeepQN shape")
        if int(episodes) < 1:
            raise ValueError(f"{what}: episodes {episodes} (at least 1)")
        if int(points_to_win) < 1:
            raise ValueError(f"{what}: points_to_win must be at least 1, not {points_to_win}")
        if credit not in CREDITS:
            raise ValueError(f"{what}: credit is one of {CREDITS}, not {credit!r}")
        from .deepqn import DeepQNHalf
        self.C, self.n_actions, E = int(C), int(n_actions), int(episodes)
        half, tiled = precision == "float16", fc1_layout == "tiled"
        P = dqn_params(self.C, self.n_actions)
        self._params = dict.fromkeys(ROLES2, P)
        lists, scripted, flats = {"first_0": first, "second_0": second}, {}, {}
        for role, seats in lists.items():
            if seats is None or len(seats) == 0:
                raise ValueError(f"{what}: no seat for role {role}")
            if any(isinstance(x, MLPBaseline) for x in seats):
                raise ValueError(f"{what}: an MLPBaseline is a simple_adversary policy, not a duel seat")
            kinds = {_is_seat(x) for x in seats}
            if len(kinds) != 1:
                raise ValueError(f"{what}: role {role} mixes nets and scripted seats (a list holds one kind)")
            scripted[role] = kinds.pop()
        if all(scripted.values()):
            raise ValueError(f"{what}: both sides are scripted: no net to evaluate")
        for role, seats in lists.items():
            if scripted[role]:
                for i, b in enumerate(seats):
                    _check_seat(f"{what}: seat {i} of role {role}", b, self.n_actions)
                continue
            flats[role] = []
            for i, x in enumerate(seats):
                model = getattr(x, "model", x)
                if callable(getattr(model, "flat", None)) and isinstance(model, DeepQNHalf) != half:
                    raise ValueError(f"{what}: net {i} of role {role} is a {'float16' if not half else 'float32'} net in a "
                                     f"{precision} table")
                f = _flat(x)
                if f.size != P:
                    raise ValueError(f"{what}: net {i} of role {role} has {f.size} parameters, not {P}")
                flats[role].append(f)
        A, B = len(first), len(second)
        if A * B * E > MAX_GAMES:
            raise ValueError(f"{what}: {A * B * E} games (at most {MAX_GAMES})")
        self.episodes, self.precision, self.device, self.T = E, precision, device, int(limit)
        self.points_to_win, self.credit = int(points_to_win), credit
        self.net_roles = tuple(r for r in ROLES2 if not scripted[r])
        self.script_role = next((r for r in ROLES2 if scripted[r]), None)
        # ---- the slab of the nets, as DQNCrossPlay keeps it
        sym = "coevo_dqn16" if half else "coevo_dqn"
        stride = int(getattr(L.load(), sym + "_slab_stride")(self.C, self.n_actions))
        if half:   # the tiled fp16 slab has entry points of its own, the float32 one a bit in the channel argument
            pack, net_args = (sym + "_pack_tiled", sym + "_unpack_tiled") if tiled else (sym + "_pack", sym + "_unpack"), self.C
        else:
            pack, net_args = (sym + "_pack", sym + "_unpack"), self.C | (L.DQN_FC1_TILED if tiled else 0)
        self.counts = {r: len(flats.get(r, ())) for r in ROLES2}
        self.io = _CrossSlab(ROLES2, self.counts, dict.fromkeys(ROLES2, stride), self._params,
                             torch.int32 if half else torch.float32, pack, lambda r: (net_args, self.n_actions), device)
        keep = [self.io.upload(r, "cross", 0, np.stack(flats[r])) for r in self.net_roles]
        torch.cuda.current_stream().synchronize()
        del keep
        duel = dict(points_to_win=self.points_to_win, credit=credit)
        if self.script_role is None:
            from .duel_rollout import DuelRollout, HalfDuelRollout
            table = NetTable(self.io.base, dict.fromkeys(ROLES2, stride), None)
            games, episode = cross_games2(table, A, B, E)
            self._episode = np.asarray(episode, dtype=np.int64)
            self.ro = (HalfDuelRollout if half else DuelRollout)(games, table.net_off, self._episode, self.C, self.n_actions,
                                                                 self.io.slab, env_seed, 0, device, fc1_tiled=tiled, **duel)
        else:
            g = np.arange(A * B * E, dtype=np.int64)
            index = {"first_0": g // (B * E), "second_0": (g // E) % B}
            self._episode = g % E
            net_role = self.net_roles[0]
            net_off = [self.io.base[net_role]["cross"] + i * stride for i in range(self.counts[net_role])]
            table = np.stack([seat_words(b) for b in lists[self.script_role]])[index[self.script_role]]
            self.ro = (HalfDuelSeatRollout if half else DuelSeatRollout)(index[net_role], net_off, ROLES2.index(self.script_role),
                                                                         table, self._episode, self.C, self.n_actions,
                                                                         self.io.slab, env_seed, device, fc1_tiled=tiled, **duel)
        self._reduce_buffers((A, B, 1))

    def upload(self, role, i, flat):
        if role in ROLES2 and role not in self.net_roles:
            raise ValueError(f"{type(self).__name__}: role {role!r} is scripted: it has no weights")
        super().upload(role, i, flat)

    def run(self, first_ordinal):
        _check_first_ordinal(type(self).__name__, first_ordinal, lambda: self.episodes, 63)
        ro = self.ro
        ro.status.zero_()
        ro.ordinal0.copy_(torch.from_numpy(int(first_ordinal) + self._episode))
        ro.set_limits(np.full(ro.n_games, self.T, dtype=np.int32))
        ro.enqueue(self.T, None)
        torch.cuda.synchronize()
        L.raise_on_status(ro.status)
        self._reduce(ro.acc, marg_c=False)   # acc is [n][3] with a zero third column: C = 1
        A, B, _ = self.dims
        E = self.episodes
        marg = {r: self.marg[k].cpu().numpy()[:, :2] for k, r in enumerate(ROLES2)}
        words = ro.dstate.cpu().numpy().reshape(A, B, E, STATE_WORDS)
        return DuelCrossPlayResult(self.payoff.cpu().numpy().reshape(A, B, 3)[..., :2], marg,
                                   ro.acc.cpu().numpy().reshape(A, B, E, 3)[..., :2],
                                   words[..., 7:9].astype(np.int64), words[..., 11].astype(np.int64))


# ---------------------------------------------------------------------------------------------------- main.py --test
def _duel_env_or_raise(env):
    if not (isinstance(env, DuelAEC) and env.seed_value is not None):
        raise ValueError("duel cross-play runs on this package's seeded duel env (DuelAEC, initialize_env with "
                         "coevo_atari_env=\"duel\"), not on another env")


def _loaded_net(args, env):
    from .io_utils import load_agent_for_testing
    loaded = load_agent_for_testing(args, env)
    if loaded is None:
        raise ValueError(f"Unsupported algorithm for testing: {args.algorithm}")
    return (loaded[0] if isinstance(loaded, (tuple, list)) else loaded).model


def duel_test_agents(env, args, episodes=10, opponent=None):
    """``crossplay.test_agents`` for a seeded ``DuelAEC``: ``load_agent_for_testing``, then `episodes` evaluation games as ONE
    rollout under the reset ordinals that many play_game calls would have taken from `env` (its ``n_resets`` moves on by
    `episodes`); points_to_win and the credit rule are the env object's.  ``args.play_against_yourself``: the loaded agent plays
    both seats; or ``opponent``, a duel seat (``TrackerSeat()``, ``RandomBaseline()``, ...) that plays second_0 against it.
    -> ((first_0, second_0) mean returns - bit for bit the sums and the division of main.py's loop over play_game -,
    (first_0, second_0) mean points).  Under credit "next" the higher return belongs to the side that conceded more."""
    from .deepqn import DeepQN, DeepQNHalf
    from .game_logic import ATARI_GAMES
    if args.game not in ATARI_GAMES:
        raise ValueError(f"Unsupported game type: {args.game}")
    _duel_env_or_raise(env)
    if opponent is not None and not _is_seat(opponent):
        raise ValueError("duel_test_agents: `opponent` is a duel seat (TrackerSeat, RandomBaseline, PeriodicBaseline, "
                         "ConstantBaseline)")
    if opponent is None and not getattr(args, "play_against_yourself", False):
        raise ValueError("duel_test_agents: args.play_against_yourself or an `opponent` seat")
    if _eval_limit(args) is None:
        raise ValueError("duel_test_agents: the device route of the duel env plays a fixed number of launches: "
                         "args.max_evaluation_steps is required")
    net = _loaded_net(args, env)
    cp = DuelCrossPlay([net], [net] if opponent is None else [opponent], env.C, env.n_actions, episodes=episodes,
                       limit=_eval_limit(args), points_to_win=env.points_to_win, credit=env.credit,
                       precision=_precision_of((net,), DeepQNHalf, DeepQN), env_seed=env.seed_value)
    res = cp.run(_take_ordinals(env, episodes))
    return (tuple(float(v) for v in res.payoff[0, 0]), tuple(float(v) for v in res.points[0, 0].mean(axis=0)))


def duel_cross_play_checkpoints(env, args, paths_by_role, episodes=10, first_ordinal=None):
    """``crossplay.cross_play_checkpoints`` for a seeded ``DuelAEC``: ``paths_by_role`` {"first_0": path, "second_0": path}
    names whole Hall-of-Fame checkpoints (pickled Agent lists or their ``.state_dict.pth`` twins); every member plays, oldest
    first -> the ``DuelCrossPlayResult`` of evaluation games (``args.max_evaluation_steps``) from ``first_ordinal`` (default: the
    next resets of `env`, which are then taken)."""
    from .deepqn import DeepQN, DeepQNHalf
    from .io_utils import STATE_DICT_SUFFIX, agents_from_state_dicts, load_agents
    if set(paths_by_role) != set(ROLES2):
        raise ValueError(f"duel_cross_play_checkpoints: one path for each of {ROLES2}, not {sorted(paths_by_role)}")
    _duel_env_or_raise(env)
    nets = {}
    for r in ROLES2:
        path = paths_by_role[r]
        got = agents_from_state_dicts(env, args, None, path) if str(path).endswith(STATE_DICT_SUFFIX) else load_agents(path)
        nets[r] = [a.model for a in (got if isinstance(got, (list, tuple)) else [got])]
    if first_ordinal is None:
        first_ordinal = _take_ordinals(env, episodes)
    every = [m for r in ROLES2 for m in nets[r]]
    cp = DuelCrossPlay(nets["first_0"], nets["second_0"], env.C, env.n_actions, episodes=episodes, limit=_eval_limit(args),
                       points_to_win=env.points_to_win, credit=env.credit, precision=_precision_of(every, DeepQNHalf, DeepQN),
                       env_seed=env.seed_value)
    return cp.run(first_ordinal)
