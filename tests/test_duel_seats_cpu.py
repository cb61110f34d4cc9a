"""The duel's scripted seats without a GPU: the tracker's closed form against the host tracker on rendered frames (exhaustive),
``duel_seat_action`` against ``baselines.scripted_action``, ``DuelSeatRef`` (tests/duel_seat_cases.py) against the host loop on a
``DuelAEC``, the ninth header and its binding, the host-side refusals of the three entry points, and every ValueError of
``duel_crossplay`` with the library unloadable."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import coevonet_amd
from coevonet_amd import atari_duel as ad
from coevonet_amd import duel_crossplay as dx
from coevonet_amd import lib as L
from coevonet_amd.baselines import (ConstantBaseline, MLPBaseline, PeriodicBaseline, RandomBaseline, mlp_params,
                                    scripted_action)
from coevonet_amd.crossplay import MAX_GAMES, dqn_params
from coevonet_amd.game_logic import _play_atari_aec
from tests import duel_cases as dc
from tests import duel_seat_cases as sc
from tests.util import Bag

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEATS = ("coevo_dqn16_out_duel_seat_step", "coevo_dqn_out_duel_seat_step", "coevo_duel_seat_step")


# ---------------------------------------------------------------------------------------------------------------- seats
def test_tracker_closed_form_equals_the_host_tracker_on_the_rendered_frame():
    """both players, bx within 2 of the player's column or 41, by 0 .. 82, p 0 .. 72: 72 708 cases, the ball hiding paddle rows
    among them"""
    n = hidden = 0
    for s, X in ((0, ad.X0), (1, ad.X1)):
        for bx in sorted({X - 2, X - 1, X, X + 1, X + 2, 41}):
            for by in range(83):
                for p in range(73):
                    w = ad.snapshot_word(bx, by, p if s == 0 else 36, p if s == 1 else 36)
                    frame = ad.render_frame([0, 0, 0, w], s, 4)
                    assert dx.duel_tracker_word(w, s) == ad.duel_tracker_action(frame, s), (s, bx, by, p)
                    n += 1
                    hidden += bx <= X <= bx + 1 and by < p <= by + 1
    assert n == 72708 and hidden > 0      # (hidden: the ball covers paddle row p itself - the min(p, by) branch decides)


def test_seat_action_equals_scripted_action_and_the_tracker_word():
    for n in (3, 6, 18):
        for seat in (RandomBaseline(0), RandomBaseline(2 ** 64 - 1), PeriodicBaseline(0), PeriodicBaseline(7), ConstantBaseline(2)):
            for ordinal in (0, 5, 2 ** 63 - 1):
                for parity in (0, 1):
                    for k in (0, 1, 2, 99):
                        assert dx.duel_seat_action(seat, 0x24241029, ordinal, parity, k, n) == \
                            scripted_action(seat.kind, seat.arg, seat.seed, ordinal, parity, k, n)
    w = ad.snapshot_word(41, 70, 10, 64)
    assert dx.duel_seat_action(dx.TrackerSeat(), w, 3, 0, 4, 6) == dx.duel_tracker_word(w, 0) == 3
    assert dx.duel_seat_action(dx.TrackerSeat(), w, 3, 1, 4, 2) == dx.duel_tracker_word(w, 1) == 0      # (d = 142 - 140)
    for bad in (sc.raw_seat(4), sc.raw_seat(-1), sc.raw_seat(sc.PERIODIC, -1), sc.raw_seat(sc.CONSTANT, 6), sc.raw_seat(sc.CONSTANT, -1)):
        assert sc.seat_plays(bad, w, 0, 0, 0, 6) == (0, False)
    assert sc.seat_table([sc.raw_seat(sc.RANDOM, 0, 2 ** 64 - 1), sc.raw_seat(3)]).tolist() == [[0, 0, -1, -1], [3, 0, 0, 0]]
    assert dx.TRACKER == 3 and dx.SEAT_WORDS == 4


@pytest.mark.parametrize("credit", ["next", "own"])
@pytest.mark.parametrize("script_parity", [0, 1])
@pytest.mark.parametrize("seat", [dx.TrackerSeat(), RandomBaseline(5), PeriodicBaseline(1), ConstantBaseline(3)], ids=repr)
def test_seat_ref_equals_the_host_loop(seat, script_parity, credit):
    """DuelSeatRef driven through a rollout's schedule = _play_atari_aec on a DuelAEC with ScriptedPlayer words on the net's side
    and DuelTracker / a scripted_action player on the seat's: returns, final words"""
    n, C, points = 6, 4, 2
    rng = np.random.default_rng([script_parity, len(credit)])
    scored = 0
    for ordinal, T in [(1, 1), (2, 2), (3, 3)] + [(o, 30) for o in range(4, 14)]:
        words = [int(a) for a in rng.choice([0, 1, 2, 3, 4, 5, -1, n, 255], size=T)]
        env = dc.env_at(ordinal, channels=C, points_to_win=points, credit=credit)
        env.reset()
        host_seat = ad.DuelTracker(script_parity) if isinstance(seat, dx.TrackerSeat) else sc.SeatPlayer(seat, env, script_parity, n)
        players = [dc.ScriptedPlayer(words), host_seat] if script_parity else [host_seat, dc.ScriptedPlayer(words)]
        want = _play_atari_aec(env, players[0], players[1], Bag(game="pong_v3", max_timesteps_per_episode=T), False)
        ref = sc.DuelSeatRef([ordinal], [T], None, 0, C, n, dc.SEED, [seat], script_parity, points=points, own=credit == "own")
        sc.play_ref(ref, T, words)
        assert tuple(ref.acc[0, :2]) == tuple(float(x) for x in want), (T, ref.acc[0], want)
        assert np.array_equal(ref.state[0], env.state.words()) and ref.status == 0, T
        scored += sum(env.state.score)
    assert scored > 0


# ------------------------------------------------------------------------------------------------ header, library, binding
def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def test_seat_symbols_are_declared_exported_and_bound():
    text = header_text("coevo_duel_seats.h")
    assert sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", text))) == sorted(SEATS) == L.duel_seats_symbols()
    assert "typedef" not in text and "struct" not in text
    lib, dll = L.load(), ctypes.CDLL(L.LIB_PATH)
    for name in SEATS:
        assert hasattr(dll, name), f"{name} is not exported by libcoevo.so"
        res, args = L._DUEL_SEATS_SIGS[name]
        assert res is ctypes.c_int and getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    # coevo_duel_step's arguments with (seats, script_parity) behind the limits, script_actions behind actions_prev and, in the
    # plain form, the status word in front of the stream
    p, i = ctypes.c_void_p, ctypes.c_int
    for seat, duel in (("coevo_duel_seat_step", "coevo_duel_step"), ("coevo_dqn_out_duel_seat_step", "coevo_dqn_out_duel_step"),
                       ("coevo_dqn16_out_duel_seat_step", "coevo_dqn16_out_duel_step")):
        d = L._DUEL_SIGS[duel][1]
        want = d[:8] + [p, i] + d[8:10] + [p] + d[10:]
        if seat == "coevo_duel_seat_step":
            want = want[:-1] + [p, p]
        assert L._DUEL_SEATS_SIGS[seat][1] == want, seat
    others = (set(L._SIGS) | set(L._EXT_SIGS) | set(L._XP_SIGS) | set(L._SH_SIGS) | set(L._SH16_SIGS) | set(L._BL_SIGS)
              | set(L._GT_SIGS) | set(L._DUEL_SIGS))
    assert not set(SEATS) & others
    assert not set(L.K_DUEL_SEATS) & (set(L.K) | set(L.K_EXT) | set(L.K_XP) | set(L.K_SH) | set(L.K_BL) | set(L.K_GT) | set(L.K_DUEL))
    assert L.K_DUEL_SEATS == {"COEVO_DUEL_SEAT_WORDS": 4, "COEVO_DUEL_SEAT_TRACKER": 3}
    assert sorted(L.K_BL[k] for k in ("COEVO_BL_RANDOM", "COEVO_BL_PERIODIC", "COEVO_BL_CONSTANT")) == [0, 1, 2]
    with pytest.raises(L.CoevoError, match="declares a struct"):
        L._parse_duel_seats_header("typedef struct { int32_t n; } coevo_new;")
    for taken in ("int coevo_version(void);", "int coevo_duel_step(void);", "#define COEVO_OK 0", "#define COEVO_DUEL_THREADS 3"):
        with pytest.raises(L.CoevoError, match="repeats a name"):
            L._parse_duel_seats_header(taken)
    from coevonet_amd.build import SOURCES, _headers
    assert "duel_seats.hip" in SOURCES and any(h.endswith("coevo_duel_seats.h") for h in _headers())
    for name in ("DuelCrossPlay", "DuelCrossPlayResult", "DuelSeatRollout", "HalfDuelSeatRollout", "TrackerSeat",
                 "duel_seat_action", "duel_tracker_word", "duel_test_agents", "duel_cross_play_checkpoints"):
        assert getattr(coevonet_amd, name) is getattr(dx, name) and name in coevonet_amd.__all__


def test_the_seat_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "coevo_duel_seats.h"\nint main(void) { return coevo_version() + COEVO_DUEL_SEAT_WORDS ? 0 : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                    "-c", str(src), "-o", str(tmp_path / "hdr.o")], check=True)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """COEVO_ERR_ARG comes back before any launch, so these calls need no GPU (the pointers are never followed)"""
    lib, ERR = L.load(), L.K["COEVO_ERR_ARG"]
    buf = np.zeros(4608, dtype=np.float64)
    p = buf.ctypes.data
    p += p % 16
    ok = dict(state=p, acc=p + 1024, n_games=2, ord0=p + 2048, gen=None, per_gen=0, t=2, limit=p + 3072, seats=p + 32768,
              parity=0, row_prev=p + 4096, actions=p + 5120, script=p + 33792, row_next=p + 6144, frames=p + 8192, C=4, n_act=6,
              seed=dc.SEED, points=21, flags=0)
    tail = dict(slab=p + 16384, tasks=p + 20480, n_tasks=1, n_rows=2, ws=p + 24576)

    def step(entry="coevo_duel_seat_step", **kw):
        a = {**ok, **tail, "status": p + 28672, **kw}
        args = [a[k] for k in ok]
        if entry != "coevo_duel_seat_step":
            args += [a[k] for k in tail]
        return getattr(lib, entry)(*args, a["status"], None)

    for entry in SEATS:
        for bad in (dict(state=None), dict(acc=None), dict(ord0=None), dict(limit=None), dict(n_games=0), dict(n_games=-1),
                    dict(t=-1), dict(t=65536), dict(C=5), dict(C=3), dict(C=1), dict(C=7), dict(n_act=0), dict(n_act=33),
                    dict(points=0), dict(points=-3), dict(flags=2), dict(flags=3), dict(flags=-1), dict(flags=1 << 16),
                    dict(row_prev=None), dict(actions=None), dict(row_next=None), dict(frames=p + 8192 + 8),
                    dict(seats=None), dict(script=None), dict(status=None), dict(parity=2), dict(parity=-1),
                    dict(parity=1), dict(t=3), dict(t=1, parity=0)):
            assert step(entry, **bad) == ERR, (entry, bad)
    for entry in SEATS[:2]:
        for bad in (dict(t=0), dict(slab=None), dict(tasks=None), dict(n_tasks=0), dict(n_rows=0), dict(ws=None)):
            assert step(entry, **bad) == ERR, (entry, bad)
    assert step("coevo_dqn16_out_duel_seat_step", slab=p + 16384 + 8) == ERR
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ refusals, library unloadable
@pytest.fixture
def no_load(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", boom)


def test_duel_cross_play_refusals_come_before_the_library(monkeypatch):
    from coevonet_amd.deepqn import DeepQN, DeepQNHalf
    C, n = 4, 6
    half_net, float_net = DeepQNHalf(C, n, "float16"), DeepQN(C, n, "float32")      # (a net asks the library for its size)
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    net = np.zeros(dqn_params(C, n), dtype=np.float32)
    ok = dict(C=C, n_actions=n, episodes=2, limit=8)
    make = lambda first=(net,), second=(dx.TrackerSeat(),), **kw: dx.DuelCrossPlay(list(first), list(second), **{**ok, **kw})
    with pytest.raises(ValueError, match="MLPBaseline"):
        make(second=[MLPBaseline(np.zeros(mlp_params(10), dtype=np.float32), 10)])
    with pytest.raises(ValueError, match="mixes nets and scripted seats"):
        make(second=[dx.TrackerSeat(), net])
    with pytest.raises(ValueError, match="both sides are scripted"):
        make(first=[RandomBaseline(1)], second=[dx.TrackerSeat()])
    for bad_C in (1, 3, 5, 7):
        with pytest.raises(ValueError, match="4 or 6 channels"):
            make(C=bad_C)
    with pytest.raises(ValueError, match="step limit is required"):
        make(limit=None)
    with pytest.raises(ValueError, match="negative step limit"):
        make(limit=-1)
    with pytest.raises(ValueError, match="float16 net in a float32 table"):
        make(first=[half_net])
    with pytest.raises(ValueError, match="float32 net in a float16 table"):
        make(first=[float_net], precision="float16")
    with pytest.raises(ValueError, match="Unsupported precision"):
        make(precision="bfloat16")
    with pytest.raises(ValueError, match=f"games \\(at most {MAX_GAMES}\\)"):
        make(first=[net] * 1024, second=[dx.TrackerSeat()] * 1025, episodes=1)
    with pytest.raises(ValueError, match="credit"):
        make(credit="theirs")
    for pts in (0, -2):
        with pytest.raises(ValueError, match="points_to_win"):
            make(points_to_win=pts)
    with pytest.raises(ValueError, match="constant action 6 outside"):
        make(second=[ConstantBaseline(6)])
    with pytest.raises(ValueError, match="seat kind 9"):
        bad = dx.TrackerSeat()
        bad.kind = 9
        make(second=[bad])
    with pytest.raises(ValueError, match="periodic start"):
        bad = PeriodicBaseline(0)
        bad.arg = -1
        make(second=[bad])
    with pytest.raises(ValueError, match="parameters, not"):
        make(first=[net[:-1]])
    with pytest.raises(ValueError, match="no seat for role"):
        make(second=[])
    with pytest.raises(ValueError, match="episodes"):
        make(episodes=0)
    with pytest.raises(ValueError, match="fc1_layout"):
        make(fc1_layout="wide")
    with pytest.raises(AssertionError, match="the library was loaded"):      # a good table gets as far as the library
        make()
    with pytest.raises(AssertionError, match="the library was loaded"):
        make(first=[dx.TrackerSeat()], second=[net])


def test_duel_test_agents_refusals_and_test_agents_still_refuses_the_duel(no_load):
    from coevonet_amd import crossplay as xp
    from coevonet_amd.atari_synthetic import SyntheticAtariAEC
    env = dc.env_at(1)
    args = Bag(game="pong_v3", algorithm="GA", max_evaluation_steps=4, play_against_yourself=True, coevo_load_dir="/nonexistent")
    with pytest.raises(ValueError, match="duel env.*not built"):
        xp.test_agents(env, args, episodes=2)
    with pytest.raises(ValueError, match="duel_test_agents"):      # ... and the message names the route that is built
        xp._atari_env_or_raise(env)
    with pytest.raises(ValueError, match="duel env.*not built"):
        xp.cross_play_checkpoints(env, args, {"first_0": "a", "second_0": "b"})
    synth = SyntheticAtariAEC("pong_v3")
    synth.reset(seed=1)
    for bad_env in (synth, ad.DuelAEC("pong_v3"), object()):      # (an unseeded DuelAEC is a foreign env too)
        with pytest.raises(ValueError, match="seeded duel env"):
            dx.duel_test_agents(bad_env, args)
        with pytest.raises(ValueError, match="seeded duel env"):
            dx.duel_cross_play_checkpoints(bad_env, args, {"first_0": "a", "second_0": "b"})
    with pytest.raises(ValueError, match="play_against_yourself or an `opponent`"):
        dx.duel_test_agents(env, Bag(**dict(vars(args), play_against_yourself=False)))
    with pytest.raises(ValueError, match="`opponent` is a duel seat"):
        dx.duel_test_agents(env, args, opponent=MLPBaseline(np.zeros(mlp_params(8), dtype=np.float32), 8))
    with pytest.raises(ValueError, match="max_evaluation_steps is required"):
        dx.duel_test_agents(env, Bag(**dict(vars(args), max_evaluation_steps=None)))
    with pytest.raises(ValueError, match="Unsupported game type"):
        dx.duel_test_agents(env, Bag(**dict(vars(args), game="chess")))
    with pytest.raises(ValueError, match="one path for each of"):
        dx.duel_cross_play_checkpoints(env, args, {"first_0": "a"})
    assert env.n_resets == 1      # no refusal took an ordinal
