"""The baseline gauntlet without a GPU: the seventh header and its binding, the host-side refusals of the two entry points,
the game-table builder, every ValueError of ``Gauntlet`` and of the trainers before the library is loaded, and the metrics line
with the option off."""
import ctypes
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

import coevonet_amd
from coevonet_amd import baselines as bl
from coevonet_amd import crossplay as xp
from coevonet_amd import gauntlet as gt
from coevonet_amd import lib as L
from tests import baseline_cases as bc
from tests import gauntlet_cases as gc
from tests.util import Bag

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT = ("coevo_mlp_forward_argmax_wave", "coevo_mpe_gauntlet")


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------ header, library, binding
def test_gauntlet_symbols_are_declared_exported_and_bound():
    text = header_text("coevo_gauntlet.h")
    assert sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", text))) == sorted(GT) == L.gauntlet_symbols()
    assert "typedef" not in text and "struct" not in text
    lib, dll = L.load(), ctypes.CDLL(L.LIB_PATH)
    for name in GT:
        assert hasattr(dll, name), f"{name} is not exported by libcoevo.so"
        res, args = L._GT_SIGS[name]
        assert res is ctypes.c_int and getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    assert L._GT_SIGS["coevo_mlp_forward_argmax_wave"] == L._BL_SIGS["coevo_mlp_forward_argmax"]   # the same argument list
    others = set(L._SIGS) | set(L._EXT_SIGS) | set(L._XP_SIGS) | set(L._SH_SIGS) | set(L._SH16_SIGS) | set(L._BL_SIGS)
    assert not set(GT) & others and not set(L.K_GT) & (set(L.K) | set(L.K_EXT) | set(L.K_XP) | set(L.K_SH) | set(L.K_BL))
    assert L.K_GT == {"COEVO_GT_FC": 3, "COEVO_GT_MLP": 4, "COEVO_GT_GAME_WORDS": 16, "COEVO_GT_THREADS": 256,
                      "COEVO_GT_WAVE_ROWS": 4}
    assert sorted((bl.RANDOM, bl.PERIODIC, bl.CONSTANT, gt.GT_FC, gt.GT_MLP)) == [0, 1, 2, 3, 4]
    with pytest.raises(L.CoevoError, match="declares a struct"):
        L._parse_gauntlet_header("typedef struct { int32_t n; } coevo_new;")
    for taken in ("int coevo_version(void);", "int coevo_mlp_forward_argmax(void);", "#define COEVO_OK 0",
                  "#define COEVO_MLP_H 4", "#define COEVO_CROSSPLAY_MAX_GAMES 4"):
        with pytest.raises(L.CoevoError, match="repeats a name"):
            L._parse_gauntlet_header(taken)
    from coevonet_amd.build import SOURCES, _headers
    assert "gauntlet.hip" in SOURCES and any(h.endswith("coevo_gauntlet.h") for h in _headers())


def test_the_gauntlet_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "coevo_gauntlet.h"\nint main(void) { return coevo_version() + COEVO_GT_GAME_WORDS ? 0 : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                    "-c", str(src), "-o", str(tmp_path / "hdr.o")], check=True)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """COEVO_ERR_ARG comes back before any launch, so these calls need no GPU (the pointers are never followed)"""
    lib, ERR = L.load(), L.K["COEVO_ERR_ARG"]
    buf = np.zeros(8192, dtype=np.float64)
    p = buf.ctypes.data
    ok = dict(slab=p, slab_floats=1024, mlp=p + 4096, mlp_floats=1024, games=p + 8192, n_games=2, ordinals=p + 9000, add=0,
              state=p + 10000, limit=p + 12000, cycle_first=0, n_cycles=25, pos_first=1, obs=p + 13000, actions=p + 14000,
              status=p + 15000)

    def gauntlet(**kw):
        a = {**ok, **kw}
        return lib.coevo_mpe_gauntlet(a["slab"], a["slab_floats"], a["mlp"], a["mlp_floats"], a["games"], a["n_games"],
                                      a["ordinals"], a["add"], a["state"], a["limit"], a["cycle_first"], a["n_cycles"],
                                      a["pos_first"], a["obs"], a["actions"], a["status"], None)
    for kw in (dict(slab=None), dict(slab=p + 4), dict(mlp=None), dict(mlp=p + 4100), dict(games=None), dict(ordinals=None),
               dict(state=None), dict(limit=None), dict(obs=None), dict(actions=None), dict(status=None), dict(n_games=-1),
               dict(cycle_first=-1), dict(n_cycles=-1), dict(slab_floats=-1), dict(mlp_floats=-1),
               dict(cycle_first=2 ** 31 - 30, n_cycles=25)):
        assert gauntlet(**kw) == ERR, kw
    assert gauntlet(n_games=0) == 0 and gauntlet(n_cycles=0) == 0                 # nothing to play: OK without a launch
    assert gauntlet(mlp=None, mlp_floats=0, n_games=0) == 0                        # no policy net: no slab needed
    ok = dict(nets=p, floats=5192, tasks=p + 2048, n_tasks=1, obs=p + 4096, n_rows=4, actions=p + 8192, status=p + 9000)
    for kw in (dict(nets=None), dict(nets=p + 4), dict(floats=0), dict(tasks=None), dict(obs=None), dict(actions=None),
               dict(status=None), dict(n_tasks=-1), dict(n_rows=0)):
        a = {**ok, **kw}
        args = (a["nets"], a["floats"], a["tasks"], a["n_tasks"], a["obs"], a["n_rows"], a["actions"], None, a["status"], None)
        assert lib.coevo_mlp_forward_argmax_wave(*args) == ERR == lib.coevo_mlp_forward_argmax(*args), kw
    assert lib.coevo_mlp_forward_argmax_wave(p, 5192, p, 0, p, 4, p, None, p, None) == 0
    assert not buf.any()


# --------------------------------------------------------------------------------------------------------- the game table
@pytest.mark.parametrize("episodes", [1, 3])
def test_game_words_hold_every_kind_in_every_slot(episodes):
    matches, kinds = gc.every_kind_matches()
    plan = gt.GauntletPlan(matches, episodes)
    want, fc_floats, mlp_floats = gc.expected_words(matches, kinds, episodes)
    assert plan.words.dtype == np.int32 and plan.words.shape == (7 * episodes, 16) and np.array_equal(plan.words, want)
    assert (plan.slab_floats, plan.mlp_floats, plan.n_games, plan.n_matches) == (fc_floats, mlp_floats, 7 * episodes, 7)
    assert np.array_equal(plan.episode, np.tile(np.arange(episodes), 7)) and plan.episode.dtype == np.int64
    for s in range(3):
        assert set(plan.words[:, 4 * s]) == {0, 1, 2, 3, 4}
    assert not plan.words[:, 12:].any()
    assert all(o % 64 == 0 for o in plan.fc_off) and all(o % 4 == 0 for o in plan.mlp_off)
    # seeds 0 and 2**64 - 1 in their two words
    assert {tuple(w) for w in plan.words[plan.words[:, 4] == 0][:, 6:8]} <= {(0, 0), (-1, -1), (7, 0)}
    # a Champion takes one slot per role, shared by every match that seats it
    a0, adv = gt.Champion("agent_0"), gt.Champion("adversary_0")
    plan = gt.GauntletPlan([(a0, bl.AlwaysFire, adv), (a0, gc.fc_flat(10, 1), bl.RandomBaseline(5)), (bl.AlwaysFire, bl.AlwaysFire, adv)], 2)
    assert plan.champion_off == {"agent_0": 0, "adversary_0": 139840} and plan.fc_off == [139840 + 138816]
    assert plan.words[0, 5] == plan.words[2, 5] == 0 and plan.words[0, 1] == plan.words[4, 1] == 139840
    assert plan.words[2, 9] == 139840 + 138816 and plan.slab_floats == 2 * 139840 + 138816
    assert plan.describe() == ["Champion(agent_0) + ConstantBaseline(1) vs Champion(adversary_0)",
                               "Champion(agent_0) + fc0 vs RandomBaseline(5)",
                               "ConstantBaseline(1) + ConstantBaseline(1) vs Champion(adversary_0)"]


def test_the_reference_table_is_sixty_games():
    spec = gc.reference_spec()
    assert spec.plan.n_games == 60 and spec.plan.n_matches == 6 and spec.champion_roles() == ("agent_0", "agent_1", "adversary_0")
    assert [gt.GauntletSpec.of(dict(adversaries=[bl.AlwaysFire], episodes=2)).plan.n_games, spec.first_ordinal] == [2, 1]
    assert len(spec.names()) == 6 and spec.names()[0] == "Champion(agent_0) + Champion(agent_1) vs RandomBaseline(1)"


# ------------------------------------------------------------------------------------------------------------ refusals
def no_load():
    raise AssertionError("the library was loaded")


def test_every_gauntlet_refusal_comes_before_the_library_is_loaded(monkeypatch):
    from coevonet_amd.fcnetwork import FCNetworkHalf
    half_fc = FCNetworkHalf(10, 5)      # (its constructor may load the library: built first)
    monkeypatch.setattr(L, "load", no_load)
    f10, f8 = np.zeros(xp.fc_params(10), dtype=np.float32), np.zeros(xp.fc_params(8), dtype=np.float32)
    m10, m8 = bl.MLPBaseline(np.zeros(5189, dtype=np.float32), 10), bl.MLPBaseline(np.zeros(5061, dtype=np.float32), 8)
    r = bl.RandomBaseline()
    for matches, kw, msg in (
            ([], {}, "no match"), (None, {}, "no match"), ([(f10, f10, f8)], dict(episodes=0), "episodes 0"),
            ([(f10, half_fc, f8)], {}, "match 0, role agent_1: a float16 net"),
            ([(f10, f10, f8), (f8, f10, f8)], {}, "match 1, role agent_0: a net of 138757 parameters, not 139781"),
            ([(f10, f10, f10)], {}, "match 0, role adversary_0: a net of 139781 parameters, not 138757"),
            ([(m8, r, r)], {}, "match 0, role agent_0: a policy net of width 8, not 10"),
            ([(r, r, m10)], {}, "match 0, role adversary_0: a policy net of width 10, not 8"),
            ([(r, bl.ConstantBaseline(5), r)], {}, "match 0, role agent_1: constant action 5 outside 0 .. 4"),
            ([(r, r)], {}, "match 0 is not a trio"),
            ([(gt.Champion("agent_1"), r, r)], {}, r"match 0, role agent_0: the seat is Champion\('agent_1'\)"),
            ([(r, r, r)] * 1025, dict(episodes=1024), "1049600 games")):
        with pytest.raises(ValueError, match=msg):
            gt.Gauntlet(matches, **kw)
    with pytest.raises(ValueError, match="Champion: role 'first_0'"):
        gt.Champion("first_0")
    # a Champion run before it was set, and a first ordinal outside the stream: refused by enqueue before any launch
    g = object.__new__(gt.Gauntlet)
    g.episodes, g._champion_set = 2, {"agent_0": True, "adversary_0": False}
    with pytest.raises(ValueError, match=r"Champion\('adversary_0'\) has no weights yet"):
        g.run(1)
    for first, msg in ((-1, "negative first_ordinal -1"), (2 ** 64 - 1, "leaves the 64-bit ordinals")):
        with pytest.raises(ValueError, match=msg):
            g.enqueue(first)
    g._done = None
    with pytest.raises(ValueError, match="nothing was enqueued"):
        g.result()
    for make, msg in ((lambda: gt.GauntletSpec(), "no baseline to face"), (lambda: gt.GauntletSpec(adversaries=[f8]), "is not a baseline"),
                      (lambda: gt.GauntletSpec(agent_pairs=[(r,)]), "pairs"), (lambda: gt.GauntletSpec(adversaries=[m10]), "width 10, not 8"),
                      (lambda: gt.GauntletSpec(adversaries=[r], episodes=0), "episodes 0"),
                      (lambda: gt.GauntletSpec(adversaries=[r], first_ordinal=-1), "negative first_ordinal"),
                      (lambda: gt.GauntletSpec.of(dict(adversaries=[r], games=3)), "unknown keys"),
                      (lambda: gt.GauntletSpec.of([r]), "a GauntletSpec or a dict")):
        with pytest.raises(ValueError, match=msg):
            make()


def test_every_trainer_refusal_names_the_option_and_comes_before_the_library_is_loaded(monkeypatch):
    from coevonet_amd import dqn_population as dp
    from coevonet_amd import evolutionary_strategy as es
    from coevonet_amd import genetic_algorithm as ga
    monkeypatch.setattr(L, "load", no_load)
    spec = dict(adversaries=[bl.RandomBaseline()], episodes=2)
    rank0 = types.SimpleNamespace(rank=0, world=2, gather_ga=lambda eng: None)
    one = types.SimpleNamespace(rank=0, world=1, gather_ga=lambda eng: None)

    class Only:      # nothing else: no other attribute may be read before the refusal
        def __init__(self, **kw):
            self.__dict__.update(kw)
    cases = [(Only(precision="float16"), {}, "float32 training only"), (Only(precision="float16"), dict(rng="device_philox"), "float32"),
             (Only(), dict(dist_ctx=rank0), "one rank only"), (Only(), dict(dist_ctx=one), "one rank only"),
             (Only(), dict(env_mode="host"), 'not env "host"'), (Only(coevo_env="host"), {}, 'not env "host"'),
             (Only(), dict(rng="device_philox"), "coevo_device_loop = False"),
             (Only(coevo_rng="device_philox", coevo_device_loop=True), {}, "coevo_device_loop = False")]
    for args, kw, msg in cases:
        for call in (lambda: ga.GATrainer(None, args, gauntlet=spec, **kw),
                     lambda: ga.genetic_algorithm_train(None, None, args, None, gauntlet=spec, **kw)):
            with pytest.raises(ValueError, match=msg) as e:
                call()
            assert "coevo_gauntlet" in str(e.value)
        args.coevo_gauntlet = spec          # the option on the args bag is the same option
        with pytest.raises(ValueError, match=msg):
            ga.GATrainer(None, args, **kw)
    with pytest.raises(ValueError, match="coevo_gauntlet: no baseline to face"):
        ga.GATrainer(None, Only(coevo_gauntlet={}))
    with pytest.raises(ValueError, match="coevo_gauntlet: a GauntletSpec or a dict"):
        ga.GATrainer(None, Only(coevo_gauntlet=[bl.AlwaysFire]))
    on = Only(coevo_gauntlet=spec)
    for call in (lambda: es.ESTrainer(None, on), lambda: es.evolution_strategy_train(None, on, None),
                 lambda: dp.DQNGATrainer(None, on), lambda: dp.DQNESTrainer(None, on),
                 lambda: dp.dqn_genetic_algorithm_train(None, None, on, None), lambda: dp.dqn_evolution_strategy_train(None, on, None)):
        with pytest.raises(ValueError, match="args.coevo_gauntlet: the baseline gauntlet is not built for") as e:
            call()
        assert "ES" in str(e.value) or "DeepQN" in str(e.value)
    with pytest.raises(ValueError, match="not built for the DeepQN trainers"):
        ga.genetic_algorithm_train(None, None, Only(game="pong_v3"), None, gauntlet=spec)


def test_public_surface():
    for name in ("Gauntlet", "Champion", "GauntletResult", "GauntletSpec"):
        assert getattr(coevonet_amd, name) is getattr(gt, name) and name in coevonet_amd.__all__
    assert gt.fc_stride(10) == 139840 == L.load().coevo_fc_slab_stride(10) and gt.fc_stride(8) == 138816 == L.load().coevo_fc_slab_stride(8)


# ------------------------------------------------------------------------------------------------------------ the JSONL line
def test_the_metrics_line_has_no_gauntlet_key_with_the_option_off(tmp_path, monkeypatch):
    """genetic_algorithm_train's writer over a stub trainer: the line of today with the option off, + "gauntlet" with it on"""
    from coevonet_amd import genetic_algorithm as ga

    class StubTrainer:
        device_loop = sharded_loop = False

        def __init__(self, env, args, gauntlet=None, **kw):
            self.res, self.gen, self.gauntlet = ga.GAResult(), 0, gauntlet
            if gauntlet is not None:
                self.res.gauntlet = []

        def step(self):
            for r in ga.ROLES:
                self.res.rewards[r].append(-1.0 - self.gen)
            self.res.sigma_after.append([0.05] * 3)
            self.res.seconds.append(0.5)
            if self.gauntlet is not None:
                self.res.gauntlet.append([[-2.0, -2.0, -3.0 - self.gen]])
            self.gen += 1

        def finish(self):
            return self.res
    monkeypatch.setattr(ga, "GATrainer", StubTrainer)
    off, on = tmp_path / "off", tmp_path / "on"
    ga.genetic_algorithm_train(None, None, Bag(generations=2), str(off))
    ga.genetic_algorithm_train(None, None, Bag(generations=2), str(on), gauntlet=object())
    lines_off = [json.loads(x) for x in open(off / "metrics.jsonl")]
    lines_on = [json.loads(x) for x in open(on / "metrics.jsonl")]
    keys = ["generation", "eval_rewards", "mutation_power", "diversity", "elite_ids", "fitness_best", "seconds"]
    assert [list(x) for x in lines_off] == [keys, keys] and [list(x) for x in lines_on] == [keys + ["gauntlet"]] * 2
    assert lines_on[1]["gauntlet"] == [[-2.0, -2.0, -4.0]]
    assert [{k: x[k] for k in keys} for x in lines_on] == lines_off
