"""The paddle duel without a GPU: the rules against the issue's known answers and invariants, ``DuelAEC`` through the host loop
against a straight-line restatement of the books for both credit rules, the scripted players, the eighth header and its binding,
the host-side refusals of the three entry points, and every ValueError of the engines, trainers and cross-play with the library
unloadable."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from coevonet_amd import atari_duel as ad
from coevonet_amd import lib as L
from coevonet_amd.atari_synthetic import SyntheticAtariAEC
from coevonet_amd.game_logic import _play_atari_aec, initialize_env, play_game
from tests import duel_cases as dc
from tests.util import Bag

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUEL = ("coevo_dqn16_out_duel_step", "coevo_dqn_out_duel_step", "coevo_duel_step")


# ---------------------------------------------------------------------------------------------------------------- rules
def test_serve_known_answers():
    for (seed, o, k), want in dc.SERVES:
        assert ad.duel_serve(seed, o, k) == want, (seed, o, k)


def test_whole_game_known_answer():
    g = ad.DuelGame(dc.SEED, 1, 6)
    first_point = None
    for w in range(1, 41):
        g.step(3)
        g.step(2)
        if first_point is None and any(g.score):
            first_point = (w, (g.bx, g.by, g.vx, g.vy, *g.p), tuple(g.cum))
    assert first_point == (12, (41, 44, -3, 2, 72, 0), (1, -1))
    assert g.score == [2, 1] and (g.bx, g.by, g.vx, g.vy, *g.p) == (53, 45, 3, 2, 72, 0) and g.t == 80 and not g.ended


def test_invariants_random_and_tracker_players():
    """200 ordinals x 100 world steps at the reference seed: two random players score 2-8 points a game, about evenly; tracker
    against tracker never concedes; the ball never leaves [0, 82]^2"""
    totals, per_game = [0, 0], []
    rng = np.random.default_rng(0)      # (the generator seed was chosen on the CPU: some seeds give a game of 0 or 1 points)
    for o in range(200):
        g = ad.DuelGame(dc.SEED, o, 6)
        acts = rng.integers(6, size=200)
        for i in range(100):
            g.step(int(acts[2 * i]))
            g.step(int(acts[2 * i + 1]))
            assert 0 <= g.bx <= 82 and 0 <= g.by <= 82 and g.vx in (-3, 3) and -3 <= g.vy <= 3
            assert 0 <= g.p[0] <= 72 and 0 <= g.p[1] <= 72
        per_game.append(sum(g.score))
        totals = [totals[0] + g.score[0], totals[1] + g.score[1]]
    assert 2 <= min(per_game) and max(per_game) <= 8, (min(per_game), max(per_game))
    assert abs(totals[0] - totals[1]) < 0.15 * sum(totals), totals
    for o in range(200):
        env = dc.env_at(o)
        env.reset()
        assert env.ordinal == o
        for _ in range(100):
            env.step(ad.duel_tracker_action(env.observe("first_0"), 0))
            env.step(ad.duel_tracker_action(env.observe("second_0"), 1))
            assert 0 <= env.state.bx <= 82 and 0 <= env.state.by <= 82
        assert env.state.score == [0, 0], o


def test_constant_actions_score_within_fifteen_world_steps():
    """what makes 30 agent-steps enough for the engine tests: most ordinals see a point"""
    n = 0
    for o in range(200):
        g = ad.DuelGame(dc.SEED, o, 6)
        for _ in range(15):
            g.step(3)
            g.step(2)
        n += any(g.score)
    assert 160 <= n <= 180, n


@pytest.mark.parametrize("name,words,actions,want", dc.crafted(), ids=[c[0] for c in dc.crafted()])
def test_crafted_states(name, words, actions, want):
    ref = dc.DuelRef([3], [100], None, 0, 4, 6, dc.SEED)
    ref.step(0, None, None, None, None)
    ref.poke(0, **words)
    ref.step(1, [0], [actions[0]], None, None)
    ref.step(2, [0], [actions[1]], None, None)
    g = ref.games[0]
    got = dict(bx=g.bx, by=g.by, vx=g.vx, vy=g.vy, p0=g.p[0], p1=g.p[1], score0=g.score[0], score1=g.score[1])
    assert {k: got[k] for k in want} == want, (name, got)
    if "score0" in want or "score1" in want:     # a point is followed by serve 1
        assert (g.bx, g.by, g.vx, g.vy) == ad.duel_serve(dc.SEED, 3, 1) and g.cum == [want.get("score0", 0) - want.get("score1", 0),
                                                                                      want.get("score1", 0) - want.get("score0", 0)]


def test_actions_outside_the_space_move_nothing():
    for n in (6, 18):
        for a in (-1, n, 255, 2 ** 31 - 1, -2 ** 31):
            assert ad.duel_move(36, a, n) == 36, (n, a)
        assert [ad.duel_move(36, a, n) for a in range(6)] == [36, 36, 32, 40, 32, 40]
    assert [ad.duel_move(36, a, 18) for a in range(6, 18)] == [36, 36, 32, 40, 32, 40] * 2
    assert ad.duel_move(2, 2, 6) == 0 and ad.duel_move(70, 3, 6) == 72


def test_render_and_observation_planes():
    env = dc.env_at(1, channels=6)
    env.reset()
    f0 = env.observe("first_0")
    assert f0.shape == (84, 84, 6) and f0.dtype == np.uint8
    for c in range(1, 4):
        assert np.array_equal(f0[:, :, c], f0[:, :, 0])      # after reset all four planes are the initial frame
    assert (f0[:, :, 4] == 255).all() and (f0[:, :, 5] == 0).all()
    f1 = env.observe("second_0")
    assert np.array_equal(f1[:, :, :4], f0[:, :, :4]) and (f1[:, :, 4] == 0).all() and (f1[:, :, 5] == 255).all()
    p = f0[:, :, 0]
    assert (p[36:48, 4:6] == 160).all() and (p[36:48, 78:80] == 160).all() and (p[68:70, 41:43] == 255).all()
    assert int((p == 160).sum()) == 48 and int((p == 255).sum()) == 4 and int((p != 0).sum()) == 52
    frames = [p]
    for _ in range(5):
        env.step(3)
        assert np.array_equal(env.observe("second_0")[:, :, :4], env.observe("first_0")[:, :, :4])
        env.step(2)
        frames.append(env.observe("first_0")[:, :, 3])
        got = env.observe("first_0")
        for c in range(4):                                   # oldest first; plane 3 is the frame after the latest world step
            assert np.array_equal(got[:, :, c], frames[max(len(frames) - 4 + c, 0)])
    # the ball wins where it overlaps a paddle
    assert ad.render_plane(ad.snapshot_word(4, 40, 36, 36))[40, 4] == 255 and ad.render_plane(ad.snapshot_word(4, 40, 36, 36))[42, 4] == 160
    with pytest.raises(ValueError, match="4 or 6"):
        ad.DuelAEC("pong_v3", channels=5)
    with pytest.raises(ValueError, match="points_to_win"):
        ad.DuelAEC("pong_v3", points_to_win=0)
    with pytest.raises(ValueError, match="credit"):
        ad.DuelAEC("pong_v3", credit="mine")
    with pytest.raises(ValueError, match="Unsupported game"):
        ad.DuelAEC("tennis_v3")
    assert not isinstance(env, SyntheticAtariAEC) and not issubclass(ad.DuelAEC, SyntheticAtariAEC)


# ------------------------------------------------------------------------------------------------ the books, host loop
@pytest.mark.parametrize("credit", ["next", "own"])
@pytest.mark.parametrize("game,points", [("pong_v3", 21), ("boxing_v2", 2), ("pong_v3", 1)])
def test_host_loop_against_the_straight_line_books(credit, game, points):
    """play_game with scripted players through _play_atari_aec (the host loop as it stands) = books(), for several limits, a
    game that ends by points, and what the env object holds afterwards"""
    n = ad.ATARI_GAMES[game]
    rng = np.random.default_rng(5)
    seen_points = 0
    for ordinal, T in [(1, 1), (2, 2), (3, 3), (4, 30), (5, 61), (6, 200), (7, 400)]:
        acts = [int(a) for a in rng.integers(-1, n + 1, size=T)]
        env = dc.env_at(ordinal, game=game, points_to_win=points, credit=credit)
        args = Bag(game=game, max_timesteps_per_episode=T, max_evaluation_steps=T, coevo_host_aec=True)
        got = play_game(env=env, player1=dc.ScriptedPlayer(acts[0::2]), player2=dc.ScriptedPlayer(acts[1::2]), args=args)
        want, steps = dc.books(acts, dc.SEED, ordinal, n, points, credit)
        assert env.ordinal == ordinal and tuple(got) == want, (ordinal, T, got, want)
        assert env.t == steps and env.agent_selection == env.possible_agents[steps & 1]
        assert bool(env.state.ended) == (steps < T) or (env.state.ended == T)
        if env.state.ended:
            assert env.state.ended == steps and max(env.state.score) == points and env.last()[2]
            snap = env.snapshot()
            env.step(3)                                      # an ended game books nothing further
            assert env.snapshot() == snap
        seen_points += sum(env.state.score)
        # zero-sum: "own" is "next" negated, step for step
        other = dc.books(acts, dc.SEED, ordinal, n, points, "own" if credit == "next" else "next")[0]
        assert other == (-want[0], -want[1])
    assert seen_points >= min(points, 5)


def test_next_credit_rewards_losing():
    """first_0 never moves and loses every point against a tracker: under "next" its return is positive (the reference's rule)"""
    for credit, sign in (("next", 1), ("own", -1)):
        env = dc.env_at(1, credit=credit, points_to_win=3)
        env.reset()
        args = Bag(game="pong_v3", max_timesteps_per_episode=2000)
        r = _play_atari_aec(env, dc.ScriptedPlayer([0] * 1000), ad.DuelTracker(1), args, False)
        assert env.state.score == [0, 3] and env.state.ended
        # first_0 collects at its next step, so the last point stays uncollected by it; second_0 collects all three
        assert r == (sign * 2.0, sign * -3.0), r


def test_tracker_and_random_players():
    env = dc.env_at(2)
    env.reset()
    obs = env.observe("first_0")
    assert ad.duel_tracker_action(obs, 0) in (0, 2, 3)
    for by, p, want in ((10, 36, 2), (70, 36, 3), (41, 36, 0), (39, 36, 0), (43, 36, 0), (44, 36, 3), (38, 36, 2)):
        plane = ad.render_plane(ad.snapshot_word(41, by, p, 72 - p))
        o = np.zeros((84, 84, 4), dtype=np.uint8)
        o[:, :, 3] = plane
        assert ad.duel_tracker_action(o, 0) == want, (by, p)
    a, b = ad.DuelRandom(3), ad.DuelRandom(3)
    seq = [a.determine_action(None, None) for _ in range(50)]
    assert seq == [b.determine_action(None, None) for _ in range(50)] and set(seq) <= set(range(6)) and len(set(seq)) > 3
    assert ad.DuelTracker(1).determine_action(obs, None) in (0, 2, 3)


# ------------------------------------------------------------------------------------------------ initialize_env
def test_initialize_env_default_is_the_synthetic_env():
    for args in (Bag(game="pong_v3"), Bag(game="boxing_v2", coevo_atari_env="synthetic", coevo_channels=6)):
        env = initialize_env(args)
        assert type(env) is SyntheticAtariAEC and env.n_resets == 1
    env = initialize_env(Bag(game="pong_v3", coevo_atari_env="duel", coevo_channels=6, coevo_duel_points=5, coevo_duel_credit="own"))
    assert type(env) is ad.DuelAEC and (env.C, env.points_to_win, env.credit, env.n_resets, env.ordinal) == (6, 5, "own", 1, 0)
    assert (env.state.bx, env.state.by, env.state.vx, env.state.vy) == ad.duel_serve(dc.SEED, 0, 0)
    env = initialize_env(Bag(game="boxing_v2", coevo_atari_env="duel"))
    assert (env.C, env.n_actions, env.points_to_win, env.credit) == (4, 18, 21, "next")
    with pytest.raises(ValueError, match="coevo_atari_env"):
        initialize_env(Bag(game="pong_v3", coevo_atari_env="ale"))


# ------------------------------------------------------------------------------------------------ header, library, binding
def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def test_duel_symbols_are_declared_exported_and_bound():
    text = header_text("coevo_duel.h")
    assert sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", text))) == sorted(DUEL) == L.duel_symbols()
    assert "typedef" not in text and "struct" not in text
    lib, dll = L.load(), ctypes.CDLL(L.LIB_PATH)
    for name in DUEL:
        assert hasattr(dll, name), f"{name} is not exported by libcoevo.so"
        res, args = L._DUEL_SIGS[name]
        assert res is ctypes.c_int and getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    # coevo_synth_step's arguments with points_to_win and flags in front of the stream (and of what the fused forms add)
    for duel, synth in (("coevo_duel_step", "coevo_synth_step"), ("coevo_dqn_out_duel_step", "coevo_dqn_out_synth_step"),
                        ("coevo_dqn16_out_duel_step", "coevo_dqn16_out_synth_step")):
        s = L._SIGS[synth][1]
        assert L._DUEL_SIGS[duel][1] == s[:15] + [ctypes.c_int, ctypes.c_int] + s[15:]
    others = (set(L._SIGS) | set(L._EXT_SIGS) | set(L._XP_SIGS) | set(L._SH_SIGS) | set(L._SH16_SIGS) | set(L._BL_SIGS)
              | set(L._GT_SIGS))
    assert not set(DUEL) & others
    assert not set(L.K_DUEL) & (set(L.K) | set(L.K_EXT) | set(L.K_XP) | set(L.K_SH) | set(L.K_BL) | set(L.K_GT))
    assert L.K_DUEL == {"COEVO_DUEL_STATE_WORDS": 16, "COEVO_DUEL_NO_ACTION": 255, "COEVO_DUEL_CREDIT_OWN": 1,
                        "COEVO_DUEL_THREADS": 256}
    assert ad.STATE_WORDS == L.K_DUEL["COEVO_DUEL_STATE_WORDS"] and ad.NO_ACTION == L.K_DUEL["COEVO_DUEL_NO_ACTION"]
    assert len(L._SIGS) == 132 and len(L.STRUCTS) == 17 and len(L._EXT_SIGS) == 6      # the pinned tables are as they were
    with pytest.raises(L.CoevoError, match="declares a struct"):
        L._parse_duel_header("typedef struct { int32_t n; } coevo_new;")
    for taken in ("int coevo_version(void);", "int coevo_mpe_gauntlet(void);", "#define COEVO_OK 0", "#define COEVO_GT_FC 3"):
        with pytest.raises(L.CoevoError, match="repeats a name"):
            L._parse_duel_header(taken)
    from coevonet_amd.build import SOURCES, _headers
    assert "duel_env.hip" in SOURCES and any(h.endswith("coevo_duel.h") for h in _headers())


def test_the_duel_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "coevo_duel.h"\nint main(void) { return coevo_version() + COEVO_DUEL_STATE_WORDS ? 0 : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                    "-c", str(src), "-o", str(tmp_path / "hdr.o")], check=True)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """COEVO_ERR_ARG comes back before any launch, so these calls need no GPU (the pointers are never followed)"""
    lib, ERR = L.load(), L.K["COEVO_ERR_ARG"]
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p += p % 16
    ok = dict(state=p, acc=p + 1024, n_games=2, ord0=p + 2048, gen=None, per_gen=0, t=2, limit=p + 3072, row_prev=p + 4096,
              actions=p + 5120, row_cur=p + 6144, frames=p + 8192, C=4, n_act=6, seed=dc.SEED, points=21, flags=0)
    tail = dict(slab=p + 16384, tasks=p + 20480, n_tasks=1, n_rows=2, ws=p + 24576, status=p + 28672)

    def step(entry="coevo_duel_step", **kw):
        a = {**ok, **tail, **kw}
        args = [a[k] for k in ok]
        if entry != "coevo_duel_step":
            args += [a[k] for k in tail]
        return getattr(lib, entry)(*args, None)

    for entry in DUEL:
        for bad in (dict(state=None), dict(acc=None), dict(ord0=None), dict(limit=None), dict(n_games=0), dict(n_games=-1),
                    dict(t=-1), dict(t=65536), dict(C=5), dict(C=3), dict(C=1), dict(C=7), dict(n_act=0), dict(n_act=33),
                    dict(points=0), dict(points=-3), dict(flags=2), dict(flags=3), dict(flags=-1), dict(flags=1 << 16),
                    dict(row_prev=None), dict(actions=None), dict(row_cur=None), dict(frames=p + 8192 + 8)):
            assert step(entry, **bad) == ERR, (entry, bad)
    for entry in DUEL[:2]:
        for bad in (dict(t=0), dict(slab=None), dict(tasks=None), dict(n_tasks=0), dict(n_rows=0), dict(ws=None), dict(status=None)):
            assert step(entry, **bad) == ERR, (entry, bad)
    assert step("coevo_dqn16_out_duel_step", slab=p + 16384 + 8) == ERR
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ refusals, library unloadable
@pytest.fixture
def no_load(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", boom)


def test_engines_refuse_what_the_duel_does_not_cover(no_load):
    from coevonet_amd.dqn_es_half import HalfDQNESEngine
    from coevonet_amd.dqn_ga_half import HalfDQNGAEngine
    from coevonet_amd.dqn_population import DQNESEngine, DQNGAEngine
    ga = lambda cls, C=4, **kw: cls(3, 1, 1, C, 6, 30, 30, env="duel", **kw)
    es = lambda cls, C=4, **kw: cls(4, C, 6, 30, 30, env="duel", **kw)
    for make, cls in ((ga, DQNGAEngine), (es, DQNESEngine), (ga, HalfDQNGAEngine), (es, HalfDQNESEngine)):
        name = cls.__name__
        with pytest.raises(ValueError, match="frames"):
            make(cls, frames="host")
        with pytest.raises(ValueError, match="one rank"):
            make(cls, shard=(1, 2))
        for C in (1, 3, 5):
            with pytest.raises(ValueError, match=f"{name}: the duel env renders 4 or 6 channels"):
                make(cls, C=C)
        with pytest.raises(ValueError, match="duel_points"):
            make(cls, duel_points=0)
        with pytest.raises(ValueError, match="duel_credit"):
            make(cls, duel_credit="theirs")
        with pytest.raises(ValueError, match="env is one of"):
            (cls(3, 1, 1, 4, 6, 30, 30, env="ale") if make is ga else cls(4, 4, 6, 30, 30, env="ale"))
        with pytest.raises(AssertionError, match="the library was loaded"):    # a good duel engine gets as far as the library
            make(cls)
        with pytest.raises(AssertionError, match="the library was loaded"):    # ... and so does the default, the synthetic env
            (cls(3, 1, 1, 4, 6, 30, 30) if make is ga else cls(4, 4, 6, 30, 30))


def test_trainers_pick_the_engine_env_from_the_env_object():
    """(the trainers draw their initial nets first, which asks the library for the parameter count: no GPU is touched)"""
    from coevonet_amd.dqn_population import DQNESTrainer, DQNGATrainer
    from coevonet_amd.duel_rollout import env_option_of
    duel = dc.env_at(1, channels=6, points_to_win=7, credit="own")
    assert env_option_of(duel) == {"env": "duel", "duel_points": 7, "duel_credit": "own"}
    assert env_option_of(SyntheticAtariAEC("pong_v3")) == {} and env_option_of(object()) == {}
    for trainer, algo in ((DQNGATrainer, "GA"), (DQNESTrainer, "ES")):
        for precision in ("float32", "float16"):
            args = Bag(algorithm=algo, game="pong_v3", population=2, hof_size=1, elites_number=1, precision=precision,
                       max_timesteps_per_episode=4, max_evaluation_steps=4, coevo_frames="host")
            with pytest.raises(ValueError, match="frames"):
                trainer(duel, args)


def test_cross_play_over_the_duel_is_refused_by_name(no_load):
    from coevonet_amd import crossplay as xp
    env = dc.env_at(1)
    with pytest.raises(ValueError, match="duel env.*not built"):
        xp._atari_env_or_raise(env)
    with pytest.raises(ValueError, match="duel env.*not built"):
        xp.test_agents(env, Bag(game="pong_v3", max_evaluation_steps=4, coevo_load_dir="/nonexistent"), episodes=2)


def test_device_route_refuses_a_missing_step_limit(monkeypatch):
    from coevonet_amd.deepqn import DeepQN
    env = dc.env_at(1)
    a = DeepQN(4, 6, "float32")
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    with pytest.raises(ValueError, match="step limit"):
        play_game(env=env, player1=a, player2=a, args=Bag(game="pong_v3", max_timesteps_per_episode=None))
