"""The DeepQN rollouts over the paddle duel (``atari_duel``, include/coevo_duel.h): ``DuelRollout`` and ``HalfDuelRollout`` are
``SynthRollout`` / ``HalfSynthRollout`` - the same task tables, buffers, cohorts and forward launches - whose env-step launches
are the duel's (coevo_duel_step, coevo_dqn_out_duel_step, coevo_dqn16_out_duel_step), plus the ``[n, 16]`` int32 game state those
launches keep.  ``duel_env_option`` is what the four DeepQN engines do with their ``env=`` keyword.  Everything measured over these
rollouts is labelled duel."""
from __future__ import annotations

import torch

from . import lib as L
from .atari_duel import CREDITS, STATE_WORDS
from .dqn_ga_half import HalfSynthRollout
from .dqn_population import SynthRollout

ENVS = ("synthetic", "duel")


def duel_env_option(who, env, points, credit, C, frames="device", shard=(0, 1)):
    """the ``env`` / ``duel_points`` / ``duel_credit`` keywords of a DeepQN engine -> None for the synthetic env, or the keywords
    of a duel rollout; what the duel does not cover is a ValueError (before the library is loaded)"""
    if env not in ENVS:
        raise ValueError(f"{who}: env is one of {ENVS}, not {env!r}")
    if env == "synthetic":
        return None
    if frames != "device":
        raise ValueError(f'{who}: the duel env renders its frames on the device only, not frames="{frames}"')
    if tuple(shard) != (0, 1):
        raise ValueError(f"{who}: the duel env runs on one rank only, not shard {tuple(shard)}")
    if int(C) not in (4, 6):
        raise ValueError(f"{who}: the duel env renders 4 or 6 channels, not {C}")
    if int(points) < 1:
        raise ValueError(f"{who}: duel_points must be at least 1, not {points}")
    if credit not in CREDITS:
        raise ValueError(f"{who}: duel_credit is one of {CREDITS}, not {credit!r}")
    return {"points_to_win": int(points), "credit": credit}


def env_option_of(env_obj):
    """the engine keywords that make an engine play the env object a trainer was handed"""
    from .atari_duel import DuelAEC
    if isinstance(env_obj, DuelAEC):
        return {"env": "duel", "duel_points": env_obj.points_to_win, "duel_credit": env_obj.credit}
    return {}


class _DuelState:
    def _init_duel(self, points_to_win, credit):
        if credit not in CREDITS or int(points_to_win) < 1 or self.C not in (4, 6):
            raise ValueError(f"duel rollout: credit {credit!r}, points_to_win {points_to_win} or {self.C} channels out of range")
        self.points_to_win, self.credit = int(points_to_win), credit
        self.flags = L.K_DUEL["COEVO_DUEL_CREDIT_OWN"] if credit == "own" else 0
        self.dstate = torch.zeros(self.n_games, STATE_WORDS, dtype=torch.int32, device=self.device)


class DuelRollout(_DuelState, SynthRollout):
    """``SynthRollout`` over the duel: per agent-step coevo_dqn_out_duel_step (coevo_duel_step at t = 0) + the conv-stack and fc1
    launches of coevo_dqn_forward_hidden_timed.  ``dstate`` [n, 16] int32 is the games' state; ``gstate`` stays unused."""

    def __init__(self, *a, points_to_win=21, credit="next", **k):
        super().__init__(*a, **k)
        self._init_duel(points_to_win, credit)

    def _enqueue_lane(self, ln, T, g, stream, timed):
        g0, m = ln["g0"], ln["n"]
        gs, ac = self.dstate.data_ptr() + 4 * STATE_WORDS * g0, self.acc.data_ptr() + 24 * g0
        o0, lim = self.ordinal0.data_ptr() + 8 * g0, self.limit.data_ptr() + 4 * g0
        lib = L.load()
        for t in range(T + 1):
            p, q = t & 1, (t - 1) & 1
            if t == 0:
                L._check(lib.coevo_duel_step(gs, ac, m, o0, g, self.ordinals_per_gen, t, lim, None, None, L._p(ln["rows"][p]),
                                             L._p(ln["frames"]), self.C, self.n_actions, self.env_seed, self.points_to_win,
                                             self.flags, stream), "coevo_duel_step")
            else:   # the output layer of step t-1 rides in the env-step launch
                L._check(lib.coevo_dqn_out_duel_step(gs, ac, m, o0, g, self.ordinals_per_gen, t, lim, L._p(ln["rows"][q]),
                                                     ln["actions"][q].data_ptr(), L._p(ln["rows"][p]) if t < T else None,
                                                     L._p(ln["frames"]) if t < T else None, self.C, self.n_actions,
                                                     self.env_seed, self.points_to_win, self.flags, L._p(self.slab),
                                                     L._p(ln["tasks"][q]), ln["n_tasks"][q], m, L._p(ln["ws"]),
                                                     L._p(self.status), stream), "coevo_dqn_out_duel_step")
            if t < T:
                tc, which = None, 0
                if timed and self.timing_ctx and t % self.timing_every == 0 and not torch.cuda.is_current_stream_capturing():
                    which = (t // self.timing_every) & 1
                    tc = self.timing_ctx[which]
                L._check(lib.coevo_dqn_forward_hidden_timed(L._p(self.slab), L._p(ln["tasks"][p]), ln["n_tasks"][p],
                                                            ln["max_rows"][p], m, self.Cw, self.n_actions, L._p(ln["frames"]),
                                                            L._p(ln["ws"]), tc, which, stream),
                         "coevo_dqn_forward_hidden_timed")


class HalfDuelRollout(_DuelState, HalfSynthRollout):
    """``HalfSynthRollout`` over the duel: coevo_dqn16_out_duel_step (coevo_duel_step at t = 0) + coevo_dqn16_forward_hidden;
    ``COEVO_DQN16_FUSED_OUT=0`` keeps coevo_duel_step + coevo_dqn16_forward_argmax."""

    def __init__(self, *a, points_to_win=21, credit="next", **k):
        super().__init__(*a, **k)
        self._init_duel(points_to_win, credit)

    def enqueue_step(self, ln, t, T, g, stream):
        m, lib = ln["n"], L.load()
        p, q = t & 1, (t - 1) & 1
        env = (L._p(self.dstate), L._p(self.acc), m, L._p(self.ordinal0), g, self.ordinals_per_gen, t, L._p(self.limit),
               L._p(ln["rows"][q]) if t else None, ln["actions"][q].data_ptr() if t else None,
               L._p(ln["rows"][p]) if t < T else None, L._p(ln["frames"]) if t < T else None, self.C, self.n_actions,
               self.env_seed, self.points_to_win, self.flags)
        fwd = (L._p(self.slab), L._p(ln["tasks"][p]), ln["n_tasks"][p], ln["max_rows"][p], m, self.C, self.n_actions,
               L._p(ln["frames"]))
        if t and self.fused_out:   # the output layer of step t-1 rides in the env-step launch
            L._check(lib.coevo_dqn16_out_duel_step(*env, L._p(self.slab), L._p(ln["tasks"][q]), ln["n_tasks"][q], m,
                                                   L._p(ln["ws"]), L._p(self.status), stream), "coevo_dqn16_out_duel_step")
        else:
            L._check(lib.coevo_duel_step(*env, stream), "coevo_duel_step")
        if t < T and self.fused_out:
            L._check(getattr(lib, self._hidden_entry)(*fwd, L._p(self.status), L._p(ln["ws"]), stream), self._hidden_entry)
        elif t < T:
            L._check(getattr(lib, self._argmax_entry)(*fwd, ln["actions"][p].data_ptr(), None, L._p(self.status),
                                                      L._p(ln["ws"]), stream), self._argmax_entry)
