"""Statements for the duel's scripted seats (coevonet_amd/duel_crossplay.py, include/coevo_duel_seats.h): ``DuelSeatRef``, a
plain-Python model of one coevo_duel_seat_step launch built on tests/duel_cases.DuelRef by the header's equivalence - the launch is
coevo_duel_step(t) without frames followed by coevo_duel_step(t + 1) handed the seat's action -, the launch schedule of a
rollout, raw seat rows (invalid ones included) and host players for the AEC loop.  No GPU and no library here:
tests/test_duel_seats_cpu.py proves these against the host loop, tests/test_duel_seats_gpu.py lays the device beside them."""
from types import SimpleNamespace

import numpy as np

from coevonet_amd import duel_crossplay as dx
from coevonet_amd import lib as L
from coevonet_amd.baselines import CONSTANT, PERIODIC, RANDOM
from tests import duel_cases as dc

TRACKER = dx.TRACKER
BAD_TASK = L.K["COEVO_ST_BAD_TASK"]
FILL_SCRIPT = -77


def raw_seat(kind, arg=0, seed=0):
    """a seat row as (kind, arg, seed): what the table holds, valid or not"""
    return SimpleNamespace(kind=int(kind), arg=int(arg), seed=int(seed))


def seat_table(seats):
    """[len(seats)][4] int32: {kind, arg, seed low word, seed high word}"""
    return np.stack([dx.seat_words(s) for s in seats])


def seat_plays(seat, word15, ordinal, parity, k, n_actions):
    """-> (action, valid): an invalid seat plays 0"""
    try:
        return dx.duel_seat_action(seat, word15, ordinal, parity, k, n_actions), True
    except ValueError:
        return 0, False


class DuelSeatRef(dc.DuelRef):
    """one coevo_duel_seat_step launch after another over G games, in plain Python"""

    def __init__(self, ordinal0, limits, gen, per_gen, C, n_actions, seed, seats, script_parity, points=21, own=False):
        super().__init__(ordinal0, limits, gen, per_gen, C, n_actions, seed, points, own)
        self.seats, self.parity = list(seats), int(script_parity)
        self.script_actions = np.full(self.G, FILL_SCRIPT, dtype=np.int32)
        self.status = 0

    def seat_step(self, t, row_prev, actions, row_next, frames):
        """frames: [rows][84][84][C] uint8 to render the frames of step t + 1 into, or None -> the rows rendered"""
        assert (t & 1) == self.parity
        self.step(t, row_prev, actions, None, None)                      # coevo_duel_step(t), bookkeeping only
        for g in range(self.G):
            if t < self.lim[g] and not self.games[g].ended:
                word15 = int(self.state[g, 15]) & 0xFFFFFFFF
                a, ok = seat_plays(self.seats[g], word15, self.ordinal[g], self.parity, (t - self.parity) // 2, self.n)
                self.script_actions[g] = a
                self.status |= 0 if ok else BAD_TASK
        return self.step(t + 1, np.arange(self.G), self.script_actions, row_next, frames)   # coevo_duel_step(t + 1)


def schedule(T, script_parity):
    """the launches of a T-step rollout: [("reset", 0)] for script_parity 1, then ("seat", t) for t = parity, parity + 2, ... <= T"""
    return ([("reset", 0)] if script_parity else []) + [("seat", t) for t in range(script_parity, T + 1, 2)]


def play_ref(ref, T, net_actions):
    """drives `ref` (one game or several, every game's net playing net_actions[i] at its i-th step) through the schedule"""
    rows = np.arange(ref.G)
    for kind, t in schedule(T, ref.parity):
        if kind == "reset":
            ref.step(0, None, None, None, None)
        else:
            i = (t - 1) // 2      # the net's step t - 1 is its i-th
            acts = np.full(ref.G, net_actions[i] if t and i < len(net_actions) else -9, dtype=np.int32)
            ref.seat_step(t, rows if t else None, acts, None, None)


class SeatPlayer:
    """the host loop's seat: determine_action through duel_seat_action, on the snapshot word read back from nothing but the
    env object (kinds 0 .. 2 need no frame; the tracker's host twin is atari_duel.DuelTracker)"""

    def __init__(self, seat, env, parity, n_actions):
        self.seat, self.env, self.parity, self.n, self.k = seat, env, int(parity), int(n_actions), 0

    def determine_action(self, obs, args=None):
        a = dx.duel_seat_action(self.seat, self.env.state.hist[3], self.env.ordinal, self.parity, self.k, self.n)
        self.k += 1
        return a


__all__ = ["DuelSeatRef", "SeatPlayer", "raw_seat", "seat_table", "seat_plays", "schedule", "play_ref", "RANDOM", "PERIODIC",
           "CONSTANT", "TRACKER", "BAD_TASK", "FILL_SCRIPT"]
