"""Cache-resident population nets (COEVO_RESIDENT_MB): the budget -> which individuals' nets carry COEVO_TASK_RESIDENT, and
that the flag lands on per-individual tasks of the full device-env launch only.  No GPU: plans built with device=None."""
import numpy as np
import pytest

from coevonet_amd import genetic_algorithm as ga
from coevonet_amd import lib as L
from coevonet_amd.rollout import RolloutPlan

IND = sum(4 * L.fc_slab_stride(ga.ROLE_D[r]) for r in ga.ROLES)   # bytes of one individual's three nets


def ga_plan_inputs(pop, hof, K):
    """the game table GAEngine builds for one GPU (net ids per (region, role, i)), as (games, net_off, net_D, ids, cohort)"""
    net_off, net_D, ids = [], [], {}

    def net(region, role, i):
        key = (region, role, i)
        if key not in ids:
            ids[key] = len(net_off)
            net_off.append(1_000_000 * len(net_off))
            net_D.append(ga.ROLE_D[role])
        return ids[key]

    games = []
    for role in ga.ROLES:
        for i in range(pop):
            for k in range(hof):
                if role == "agent_0":
                    a0, a1, adv = net("pop", role, i), net("hof", "agent_1", hof - 1 - k), net("hof", "adversary_0", hof - 1 - k)
                elif role == "agent_1":
                    a0, a1, adv = net("hof", "agent_0", hof - 1 - k), net("pop", role, i), net("hof", "adversary_0", hof - 1 - k)
                else:
                    a0, a1, adv = net("hof", "agent_0", hof - 1 - k), net("hof", "agent_0", hof - 1 - k), net("pop", role, i)
                games.append((adv, a0, a1))
    for _ in range(ga.N_EVAL):
        games.append((net("hof", "adversary_0", hof - 1), net("hof", "agent_0", hof - 1), net("hof", "agent_1", hof - 1)))
    per_ind = np.repeat(ga.cohort_partition(pop, K)[1], hof)
    cohort = np.concatenate([per_ind, per_ind, per_ind, np.full(ga.N_EVAL, K - 1)]).astype(np.int32)
    return np.array(games), net_off, net_D, ids, cohort


def resident_ids(ids, pop, hof, elites, K, budget):
    bounds = ga.cohort_partition(pop, K)[0]
    n = ga.resident_prefix(budget, (hof + elites + 1) * IND, IND, bounds)
    return n, [ids[("pop", r, i)] for r in ga.ROLES for k in range(K) for i in range(bounds[k], bounds[k] + n[k])]


@pytest.mark.parametrize("mb", [0, 96, 160, 224, 256, 288, "all"])
def test_budget_is_honoured_and_split_evenly(mb):
    pop, hof, elites, K = 200, 5, 2, 2
    budget = float("inf") if mb == "all" else mb * 1e6
    n = ga.resident_prefix(budget, (hof + elites + 1) * IND, IND, ga.cohort_partition(pop, K)[0])
    assert len(n) == K and len(set(n.tolist())) == 1   # the same share in every cohort (equal cohorts)
    fixed = (hof + elites + 1) * IND
    if mb == "all":
        assert n.tolist() == [100, 100]
    else:
        used = fixed + int(n.sum()) * IND
        assert n.sum() == 0 or used <= budget
        assert int(n.sum()) + K > (budget - fixed) / IND or n[0] == 100   # one more per cohort would not fit
    if mb == 0:
        assert n.sum() == 0


def test_uneven_cohorts_and_tiny_budgets():
    assert ga.resident_prefix(5e6, 10e6, IND, [0, 3, 7]).tolist() == [0, 0]
    assert ga.resident_prefix(float("inf"), 10e6, IND, [0, 3, 7]).tolist() == [3, 4]
    assert ga.resident_prefix(10e6 + 2 * 5 * IND, 10e6, IND, [0, 3, 7]).tolist() == [3, 4]
    assert ga.resident_prefix(10e6 + 2 * 2 * IND, 10e6, IND, [0, 3, 7]).tolist() == [2, 2]


@pytest.mark.parametrize("K", [1, 2])
def test_flags_only_on_light_tasks_of_the_resident_prefix(K):
    pop, hof, elites = 40, 5, 2
    games, net_off, net_D, ids, cohort = ga_plan_inputs(pop, hof, K)
    budget = (hof + elites + 1) * IND + 2 * 7 * IND + 1
    n, res = resident_ids(ids, pop, hof, elites, K, budget)
    assert n.tolist() == ([14] if K == 1 else [7, 7])
    plan = RolloutPlan(games, net_off, net_D, device=None, heavy_rows=16, game_cohort=cohort if K > 1 else None,
                       resident_nets=res)
    assert not plan.heavy_np["reserved"].any()
    flagged = plan.light_np["reserved"] == L.TASK_RESIDENT
    assert set(np.unique(plan.light_np["reserved"]).tolist()) <= {0, L.TASK_RESIDENT}
    off_of = {v: k for k, v in ids.items()}
    got = sorted(off_of[int(o) // 1_000_000] for o in plan.light_np["net_off"][flagged])
    bounds = ga.cohort_partition(pop, K)[0]
    want = sorted(("pop", r, i) for r in ga.ROLES for k in range(K) for i in range(bounds[k], bounds[k] + n[k]))
    assert got == want
    # split evenly: every cohort's task range holds the same number of flagged tasks, per role as well
    for k in range(K):
        lb, le = plan.light_begin_np[k], plan.light_begin_np[k + 1]
        assert flagged[lb:le].sum() == 3 * n[k]


def test_budget_zero_leaves_the_task_tables_as_they_were():
    games, net_off, net_D, ids, cohort = ga_plan_inputs(30, 5, 2)
    a = RolloutPlan(games, net_off, net_D, device=None, heavy_rows=16, game_cohort=cohort)
    n, res = resident_ids(ids, 30, 5, 2, 2, 0.0)
    assert res == []
    b = RolloutPlan(games, net_off, net_D, device=None, heavy_rows=16, game_cohort=cohort, resident_nets=res)
    for x, y in ((a.light_np, b.light_np), (a.heavy_np, b.heavy_np), (a.row_game_np, b.row_game_np),
                 (a.row_slot_np, b.row_slot_np)):
        assert x.tobytes() == y.tobytes()
    assert not a.light_np["reserved"].any() and not a.heavy_np["reserved"].any()


def test_same_slab_positions_every_time():
    """the choice depends on the shape and the budget only: the same nets (slab positions) in every plan built for it"""
    games, net_off, net_D, ids, cohort = ga_plan_inputs(40, 5, 2)
    budget = 224e6
    _, r1 = resident_ids(ids, 40, 5, 2, 2, budget)
    _, r2 = resident_ids(ids, 40, 5, 2, 2, budget)
    p1 = RolloutPlan(games, net_off, net_D, device=None, heavy_rows=16, game_cohort=cohort, resident_nets=r1)
    p2 = RolloutPlan(games, net_off, net_D, device=None, heavy_rows=16, game_cohort=cohort, resident_nets=r2)
    assert p1.light_np.tobytes() == p2.light_np.tobytes()


def test_budget_from_the_environment(monkeypatch):
    monkeypatch.delenv("COEVO_RESIDENT_MB", raising=False)
    assert ga.resident_budget_bytes() == ga.RESIDENT_MB_DEFAULT * 1e6
    monkeypatch.setenv("COEVO_RESIDENT_MB", "0")
    assert ga.resident_budget_bytes() == 0
    monkeypatch.setenv("COEVO_RESIDENT_MB", "all")
    assert ga.resident_budget_bytes() == float("inf")
    monkeypatch.setenv("COEVO_RESIDENT_MB", "96")
    assert ga.resident_budget_bytes() == 96e6


@pytest.mark.parametrize("env,heavy_rows,n_local,pop,want", [
    ("device", 16, 200, 200, True),     # the full launch of the whole population
    ("host", 16, 200, 200, False),      # env on the host cores
    ("device", 32, 200, 200, False),    # the 32-row tiles (fc_cycle_kernel)
    ("device", 5, 25, 200, False),      # a rank of a sharded population: small / persistent forms
    ("device", 16, 100, 200, False),    # a rank of two
])
def test_enabled_for_the_full_device_launch_only(env, heavy_rows, n_local, pop, want):
    assert ga.resident_enabled(env, heavy_rows, n_local, pop) == want
