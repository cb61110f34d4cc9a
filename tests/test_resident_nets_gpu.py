"""Cache-resident population nets (COEVO_RESIDENT_MB) change the cache policy of loads only: a full-size Co-GA generation pair
computes the same bits with no resident net, the default budget and every net resident, and a small configuration with part
of its population resident equals the oracle port."""
import numpy as np
import pytest
import torch

from coevonet_amd import genetic_algorithm as ga
from coevonet_amd import lib as L
from coevonet_amd.game_logic import initialize_env
from oracle import ref_port as rp
from tests.util import Bag

pytestmark = pytest.mark.gpu

IND = sum(4 * L.fc_slab_stride(ga.ROLE_D[r]) for r in ga.ROLES)


def headline_args():
    """bench.py's workload: pop 200, HoF 5, elites 2, T 200, fitness sharing, adaptive sigma"""
    return Bag(algorithm="GA", generations=2, population=200, hof_size=5, game="simple_adversary_v3",
               mutation_power_agent_0=0.05, mutation_power_agent_1=0.05, mutation_power_adversary=0.05,
               learning_rate=0.1, max_timesteps_per_episode=200, max_evaluation_steps=200, elites_number=2,
               adaptive=True, max_mutation_power=0.2, min_mutation_power=0.001, fitness_sharing=True,
               early_stopping=False, patience=300, min_delta=0.1, debug=False, train=True, test=False, render=False,
               env_mode="AEC", precision="float32", save=False, average_window=50, play_against_yourself=False)


def run_headline(monkeypatch, mb, generations=2):
    if mb is None:
        monkeypatch.delenv("COEVO_RESIDENT_MB", raising=False)
    else:
        monkeypatch.setenv("COEVO_RESIDENT_MB", mb)
    torch.manual_seed(0)
    np.random.seed(0)
    args = headline_args()
    env = initialize_env(args)
    tr = ga.GATrainer(env, args, rng="device_philox", env_mode="device", collect=False)
    for _ in range(generations):
        tr.step()
    eng = tr.eng
    eng.flush_breeding()
    torch.cuda.synchronize()
    eng.ro.check_status()
    out = {"rewards": eng.ro.rewards.cpu().numpy(), "actions_by_game": eng.ro.actions_by_game.cpu().numpy(),
           "state": eng.ro.state2.cpu().numpy(), "slab": eng.slab.cpu().numpy(),
           "fitness": np.stack([eng.fitness[r].cpu().numpy() for r in ga.ROLES]),
           "order": np.stack([eng.order[r].cpu().numpy() for r in ga.ROLES]),
           "dist": eng.dist_all.cpu().numpy()}
    flagged = int((eng.plan.light_np["reserved"] == L.TASK_RESIDENT).sum())
    del tr, eng
    torch.cuda.synchronize()
    return out, flagged


def test_full_size_generations_same_bits_for_every_budget(monkeypatch):
    base, f0 = run_headline(monkeypatch, "0")
    assert f0 == 0
    for mb, want_flagged in ((None, None), ("all", 600)):
        got, f = run_headline(monkeypatch, mb)
        if want_flagged is None:   # the default budget: a part of the population, in both cohorts
            n = ga.resident_prefix(ga.RESIDENT_MB_DEFAULT * 1e6, 8 * IND, IND, ga.cohort_partition(200, 2)[0])
            want_flagged = 3 * int(n.sum())
            assert 0 < want_flagged < 600
        assert f == want_flagged, mb
        for k in base:
            assert base[k].tobytes() == got[k].tobytes(), (mb, k)


@pytest.mark.parametrize("part", ["one", "all"])
def test_small_configuration_with_resident_nets_matches_oracle_port(monkeypatch, part):
    cfg = dict(generations=3, population=6, hof_size=2, elites_number=2, max_timesteps_per_episode=30,
               max_evaluation_steps=30)
    # "one": the Hall of Fame / elite / stale nets plus a part of the individuals fit the budget, the others stream nt
    mb = "all" if part == "all" else str(((cfg["hof_size"] + cfg["elites_number"] + 1) * IND + 2.5 * IND) / 1e6)
    monkeypatch.setenv("COEVO_RESIDENT_MB", mb)
    torch.manual_seed(1)
    np.random.seed(1)
    args = Bag(algorithm="GA", **cfg)
    env = initialize_env(args)
    res = ga.genetic_algorithm_train(env, env.agents[0], args, None, rng="device_philox", env_mode="device")
    light = res.engine.plan.light_np["reserved"]
    if part == "all":
        assert (light == L.TASK_RESIDENT).sum() == 3 * cfg["population"]   # every population net (HoF nets of few rows stay nt)
    else:
        assert 0 < (light == L.TASK_RESIDENT).sum() < len(light)
    torch.manual_seed(1)
    np.random.seed(1)
    want = rp.ga_train(Bag(algorithm="GA", **cfg), noise="philox", philox_seed=0)
    pop, hof = cfg["population"], cfg["hof_size"]
    for g, w in enumerate(want):
        assert res.elite_ids[g] == w["elite_ids"], g
        got = res.game_rewards[g]
        for i in range(3 * pop * hof):
            assert list(got[i]) == w["games"][i]["rewards"], (g, i)
        assert [res.rewards[r][g] for r in ga.ROLES] == w["eval_rewards"]
