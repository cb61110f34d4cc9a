"""Float16 Atari training through the public trainers on the GPU against the CPU restatements (tests/dqn_ga16_checker.py,
tests/dqn_es16_checker.py), equalities only: ``genetic_algorithm_train`` / ``evolution_strategy_train`` with ``--game pong_v3
--precision float16`` (every reward pair, fitness, diversity, elite ids, evaluation means, sigma, every net, the env's reset
counter, metrics.jsonl), ``DQNGATrainer(collect=False)``, and the device episode route of two half players."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from coevonet_amd import dqn_population as dp
from coevonet_amd import game_logic as gl
from coevonet_amd.deepqn import DeepQNHalf
from coevonet_amd.evolutionary_strategy import evolution_strategy_train
from coevonet_amd.genetic_algorithm import genetic_algorithm_train
from coevonet_amd.population import ROLES2, adapt_mutation_power2
from tests import dqn_es16_checker as xk
from tests import dqn_ga16_checker as dk
from tests.util import Bag, sha

pytestmark = pytest.mark.gpu
PHILOX_SEED = 0x1234567890abcdef
SIGMAS = (0.05, 0.08)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_env(args, extra_resets=1):
    """initialize_env's env after `extra_resets` further resets: the trainer's games then start at ordinal 1 + extra_resets"""
    env = gl.initialize_env(args)
    for _ in range(extra_resets):
        env.reset()
    return env


# ------------------------------------------------------------------------------------------------------------------ Co-GA
# torch seeds: checked on the CPU (ga_checker_run asserts it) - sigma moves over the generations and some game credits a hit
GA_CONFIGS = {
    "pong_13_generations_adaptive": dict(game="pong_v3", C=4, n=6, pop=3, hof=2, E=2, T_train=4, T_eval=3, adaptive=True,
                                         generations=13, seed=21),
    "boxing_2_generations_fixed": dict(game="boxing_v2", C=3, n=18, pop=4, hof=1, E=1, T_train=4, T_eval=3, adaptive=False,
                                       generations=2, seed=22),
}


def ga_args(cfg):
    return Bag(game=cfg["game"], precision="float16", algorithm="GA", population=cfg["pop"], hof_size=cfg["hof"],
               elites_number=cfg["E"], max_timesteps_per_episode=cfg["T_train"], max_evaluation_steps=cfg["T_eval"],
               generations=cfg["generations"], adaptive=cfg["adaptive"], mutation_power_agent_0=SIGMAS[0],
               mutation_power_agent_1=SIGMAS[1], mutation_power_adversary=0.0, coevo_seed=PHILOX_SEED, coevo_channels=cfg["C"])


@functools.lru_cache(maxsize=None)
def ga_checker_run(name):
    """the sequential restatement from the trainer's torch seed -> (per generation the record, the final args, the final nets'
    sha256, the env the games were numbered from)"""
    cfg = GA_CONFIGS[name]
    args = ga_args(cfg)
    env = make_env(args)
    first = env.n_resets
    torch.manual_seed(cfg["seed"])
    st = dk.State(*dp.dqn_initial_population(cfg["pop"], cfg["hof"], cfg["C"], cfg["n"]))
    recs = [dk.generation(st, gen, args, cfg["E"], cfg["C"], cfg["n"], env.seed_value, philox_seed=PHILOX_SEED, first_ordinal=first)
            for gen in range(cfg["generations"])]
    shas = {r: {"pop": [sha(w) for w in st.popu[r]], "hof": [sha(w) for w in st.hof[r]], "elite": [sha(w) for w in st.elites[r]]}
            for r in ROLES2}
    assert any(any(g) for rec in recs for g in rec["games"]), "no hit was credited in any game: choose another seed"
    if cfg["adaptive"]:
        assert len({tuple(rec["sigma_after"]) for rec in recs}) == len(recs), "sigma must move in every generation"
    return recs, args, shas, first


def engine_shas(eng):
    return {r: {"pop": [sha(w) for w in eng.download(r, "pop", 0, eng.pop)], "hof": [sha(w) for w in eng.download(r, "hof", 0, eng.hof)],
                "elite": [sha(w) for w in eng.download(r, "elite", 0, eng.E)]} for r in ROLES2}


@pytest.mark.parametrize("name", list(GA_CONFIGS))
def test_float16_co_ga_training_equals_the_checker(name, tmp_path):
    cfg = GA_CONFIGS[name]
    want, want_args, want_shas, first = ga_checker_run(name)
    args = ga_args(cfg)
    env = make_env(args)
    torch.manual_seed(cfg["seed"])
    res = genetic_algorithm_train(env, None, args, str(tmp_path))
    try:
        G, n_main = cfg["generations"], 2 * cfg["pop"] * cfg["hof"]
        assert type(res.engine).__name__ == "HalfDQNGAEngine"
        assert len(res.game_rewards) == len(res.fitness) == len(res.diversity) == len(res.elite_ids) == len(res.sigma_after) == G
        for gen, rec in enumerate(want):
            assert res.game_rewards[gen].tolist() == rec["games"], (gen, "reward pairs")
            for ri, r in enumerate(ROLES2):
                assert bits(res.fitness[gen][ri]).tolist() == bits(rec["fitness"][ri]).tolist(), (gen, r, "fitness")
                assert bits(res.diversity[gen][ri]) == bits(rec["diversity"][ri]), (gen, r, "diversity")
                assert res.elite_ids[gen][ri] == [int(i) for i in rec["elite_ids"][ri]], (gen, r, "elite ids")
                assert res.rewards[r][gen] == rec["eval_rewards"][ri], (gen, r, "evaluation mean")
            assert res.sigma_after[gen] == rec["sigma_after"], (gen, "sigma")
        assert (args.mutation_power_agent_0, args.mutation_power_agent_1) == \
            (want_args.mutation_power_agent_0, want_args.mutation_power_agent_1)
        assert env.n_resets == first + G * (n_main + 10)
        assert engine_shas(res.engine) == want_shas
        lines = [json.loads(ln) for ln in open(os.path.join(str(tmp_path), "metrics.jsonl"))]
        assert lines == [dict(generation=g, eval_rewards={r: rec["eval_rewards"][ri] for ri, r in enumerate(ROLES2)},
                              mutation_power=rec["sigma_after"], elite_ids=[[int(i) for i in ids] for ids in rec["elite_ids"]],
                              data="synthetic env") for g, rec in enumerate(want)]
    finally:
        res.engine.close()


def test_float16_co_ga_trainer_without_collection():
    """collect=False: no per-generation synchronisation, nothing kept per generation - the same nets and evaluation means"""
    name = "boxing_2_generations_fixed"
    cfg = GA_CONFIGS[name]
    want, _, want_shas, first = ga_checker_run(name)
    args = ga_args(cfg)
    env = make_env(args)
    torch.manual_seed(cfg["seed"])
    tr = dp.DQNGATrainer(env, args, collect=False)
    try:
        for _ in range(cfg["generations"]):
            tr.step()
        res = tr.finish()
        assert type(tr.eng).__name__ == "HalfDQNGAEngine" and tr.half
        assert res.game_rewards == res.fitness == res.diversity == res.elite_ids == []
        for ri, r in enumerate(ROLES2):
            assert res.rewards[r] == [rec["eval_rewards"][ri] for rec in want]
        assert res.sigma_after == [rec["sigma_after"] for rec in want]
        assert engine_shas(tr.eng) == want_shas and env.n_resets == first + cfg["generations"] * (2 * cfg["pop"] * cfg["hof"] + 10)
    finally:
        tr.close()


# ------------------------------------------------------------------------------------------------------------------ Co-ES
# torch seed: chosen on the CPU so that both roles see a nonzero reward in generation 0 (es_checker_run asserts it)
ES = dict(game="pong_v3", C=4, n=6, pop=3, T=3, generations=3, seed=0, lr=0.1)


def es_args(sharing):
    return Bag(game=ES["game"], precision="float16", algorithm="ES", population=ES["pop"], max_timesteps_per_episode=ES["T"],
               max_evaluation_steps=ES["T"], generations=ES["generations"], adaptive=True, fitness_sharing=sharing,
               learning_rate=ES["lr"], mutation_power_agent_0=SIGMAS[0], mutation_power_agent_1=SIGMAS[1],
               mutation_power_adversary=0.03, coevo_seed=PHILOX_SEED, coevo_channels=ES["C"])


def es_initial_base():
    torch.manual_seed(ES["seed"])
    return {r: dk.to_half(dp.dqn_init_flat(ES["C"], ES["n"])) for r in ROLES2}


@functools.lru_cache(maxsize=None)
def es_checker_run(sharing):
    """xk.generation + the sigma rule as DQNESTrainer.step applies it -> (records, base net sha256 at the end, first ordinal)"""
    args = es_args(sharing)
    env = make_env(args)
    first = env.n_resets
    base = es_initial_base()
    rewards = {r: [] for r in ROLES2}
    recs = []
    for gen in range(ES["generations"]):
        rec = xk.generation(base, gen, (args.mutation_power_agent_0, args.mutation_power_agent_1), args.learning_rate, sharing,
                            ES["pop"], ES["C"], ES["n"], ES["T"], ES["T"], env.seed_value, philox_seed=PHILOX_SEED,
                            first_ordinal=first)
        for ri, r in enumerate(ROLES2):
            rewards[r].append(rec["eval_rewards"][ri])
        adapt_mutation_power2(args, gen, rewards, zero_adversary=False)
        rec["sigma_after"] = [args.mutation_power_agent_0, args.mutation_power_agent_1]
        recs.append(rec)
    for r in ROLES2:
        assert np.any(recs[0]["fit16"][r] != 0), (r, "no reward in generation 0: choose another torch seed")
    assert args.mutation_power_adversary == 0.03
    return recs, {r: sha(base[r]) for r in ROLES2}, first


@pytest.mark.parametrize("sharing", [False, True], ids=["plain", "sharing"])
def test_float16_co_es_training_equals_the_checker(sharing, tmp_path):
    want, want_base, first = es_checker_run(sharing)
    args = es_args(sharing)
    env = make_env(args)
    torch.manual_seed(ES["seed"])
    nets, res = evolution_strategy_train(env, args, str(tmp_path))
    try:
        G = ES["generations"]
        assert type(res.engine).__name__ == "HalfDQNESEngine"
        assert len(res.game_rewards) == len(res.fitness) == len(res.diversity) == len(res.sigma_after) == G
        for gen, rec in enumerate(want):
            assert res.game_rewards[gen].tolist() == rec["games"], (gen, "reward pairs")
            for ri, r in enumerate(ROLES2):
                assert bits(res.fitness[gen][ri]).tolist() == bits(rec["fit16"][r]).tolist(), (gen, r, "fit16")
                if sharing:
                    assert bits(res.diversity[gen][ri]) == bits(rec["score"][r]), (gen, r, "sharing score")
                else:
                    assert res.diversity[gen][ri] is None
                assert res.rewards[r][gen] == rec["eval_rewards"][ri], (gen, r, "evaluation mean")
            assert res.sigma_after[gen] == rec["sigma_after"], (gen, "sigma")
        first_base = es_initial_base()
        for ri, r in enumerate(ROLES2):
            assert nets[ri].dtype == np.float32 and sha(nets[ri]) == want_base[r] != sha(first_base[r]), (r, "base net")
            assert np.array_equal(nets[ri], dk.to_half(nets[ri])), "the returned vectors hold fp16 values"
        assert env.n_resets == first + G * (2 * ES["pop"] + 10)
        lines = [json.loads(ln) for ln in open(os.path.join(str(tmp_path), "metrics.jsonl"))]
        assert lines == [dict(generation=g, eval_rewards={r: rec["eval_rewards"][ri] for ri, r in enumerate(ROLES2)},
                              mutation_power=rec["sigma_after"], data="synthetic env") for g, rec in enumerate(want)]
    finally:
        res.engine.close()


# ---------------------------------------------------------------------------------------------------------- episode route
def test_two_half_players_play_the_episode_on_the_device(monkeypatch):
    steps = 5
    args = Bag(game="pong_v3", precision="float16", max_timesteps_per_episode=steps, max_evaluation_steps=steps - 2)
    env = gl.initialize_env(args)
    torch.manual_seed(31)
    p1, p2 = gl.create_agent(env, args), gl.create_agent(env, args)
    for p in (p1, p2):
        p.mutate(0.02)
    assert isinstance(p1.model, DeepQNHalf)
    o0 = env.n_resets   # play_game's own reset gives its game this ordinal
    want = [dk.play_game(p1.model.flat(), p2.model.flat(), 4, 6, env.seed_value, o0 + i, limit)
            for i, limit in enumerate((steps, steps - 2))]
    host = Bag(**dict(vars(args), coevo_host_aec=True))

    def no_forward(self, inputs, args):
        raise AssertionError("the AEC loop asked a half player for an action")
    with monkeypatch.context() as m:
        m.setattr(DeepQNHalf, "determine_action", no_forward)
        assert list(gl.play_game(env, p1.model, p2.model, args=args)) == want[0]
        assert list(gl.play_game(env, p1.model, p2.model, args=args, eval=True)) == want[1]
        assert env.n_resets == o0 + 2 and env.t == steps - 2 and env.agent_selection == "second_0"
        with pytest.raises(AssertionError, match="AEC loop"):   # a mixed pair keeps the AEC loop
            gl.play_atari(env, p1.model, _NoDeepQN(p2.model), args)
        with pytest.raises(AssertionError, match="AEC loop"):   # and so does args.coevo_host_aec
            gl.play_game(env, p1.model, p2.model, args=host)
        with pytest.raises(ValueError, match="step limit is required"):
            gl.play_game(env, p1.model, p2.model, args=Bag(**dict(vars(args), max_timesteps_per_episode=None)))
    # the AEC loop itself, unpatched, from the same ordinals: the same rewards, and the env object where the device route left it
    env.n_resets = o0
    assert list(gl.play_game(env, p1.model, p2.model, args=host)) == want[0]
    assert list(gl.play_game(env, p1.model, p2.model, args=host, eval=True)) == want[1]
    walked = (env.t, env.last_action, env.agent_selection, dict(env._cumulative_rewards))
    env.n_resets = o0 + 1
    assert list(gl.play_game(env, p1.model, p2.model, args=args, eval=True)) == want[1]
    assert (env.t, env.last_action, env.agent_selection, dict(env._cumulative_rewards)) == walked
    assert any(any(w) for w in want), "no hit was credited: choose another torch seed"


class _NoDeepQN:
    """a player that is no DeepQNHalf (and no DeepQN): any pair with it is a mixed pair"""

    def __init__(self, model):
        self.model = model

    def determine_action(self, inputs, args):
        return self.model.determine_action(inputs, args)
