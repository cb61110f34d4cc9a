"""The Co-GA extension modes hof_mean / population_sharing on the MI355X (include/coevo_sharing.h): the pairwise-distance
kernels, the niche counts, the fitness with its switches, GAEngine under the three non-default mode pairs and the trainer, all
as bit equalities against the numpy statements of tests/sharing_cases.py (whose inputs are order-proof: see there)."""
import json
import os

import numpy as np
import pytest
import torch

from coevonet_amd import genetic_algorithm as ga
from coevonet_amd import lib as L
from coevonet_amd.game_logic import initialize_env
from oracle import ref_port as rp
from tests import ga16_checker as gk
from tests import select_cases as sc
from tests import sharing_cases as S
from tests.util import Bag

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROLES = rp.ROLES


def bits64(t):
    return t.cpu().numpy().view(np.uint64)


def to_slab(flats, D):
    """flat parameters() vectors -> a device slab whose padding words are NaN"""
    n, stride, P = len(flats), L.fc_slab_stride(D), L.fc_param_count(D)
    slab = torch.full((n, stride), float("nan"), dtype=torch.float32, device=DEV)
    flat = torch.from_numpy(np.ascontiguousarray(flats, dtype=np.float32)).to(DEV)
    L.call("coevo_fc_pack", L._p(flat), L._p(slab), n, D)
    assert stride > P
    slab[:, P:] = float("nan")
    torch.cuda.synchronize()
    return slab


def run_pairwise(slab, n, D):
    m = int(L.load().coevo_fc_pairwise_scratch_doubles(n, D))
    scratch = torch.full((m,), float("nan"), dtype=torch.float64, device=DEV)
    dist = torch.full((n, n), float("nan"), dtype=torch.float32, device=DEV)
    L.call("coevo_fc_pairwise_distance", L._p(slab), n, D, L._p(scratch), L._p(dist))
    torch.cuda.synchronize()
    return dist, scratch


# ------------------------------------------------------------------------------------------------ pairwise distances
PAIRWISE_CASES = [("plain", n) for n in S.PAIRWISE_N] + [(k, n) for k in ("identical", "layernorm", "inf")
                                                         for n in (3, S.TILE + 1)]


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("kind,n", PAIRWISE_CASES)
def test_pairwise_distances(D, kind, n):
    assert max(S.PAIRWISE_N) <= 70
    w, want = S.crafted(D, kind, n)
    slab = to_slab(w, D)
    dist, scratch = run_pairwise(slab, n, D)
    got = dist.cpu().numpy()
    assert np.array_equal(S.bits32(got), S.bits32(want))                      # the numpy statement, every word written
    assert np.array_equal(S.bits32(got), S.bits32(got.T)) and not S.bits32(np.diag(got)).any()
    if kind == "identical":
        assert S.bits32(got[0, n - 1]) == 0 and n > 1
    if kind == "inf":
        k = n // 2
        assert np.isposinf(np.delete(got[k], k)).all() and np.isposinf(np.delete(got[:, k], k)).all()
    # a second run on the used scratch and output: the same words
    dist2, scratch2 = run_pairwise(slab, n, D)
    assert np.array_equal(S.bits32(dist2.cpu().numpy()), S.bits32(got))
    L.call("coevo_fc_pairwise_distance", L._p(slab), n, D, L._p(scratch), L._p(dist))
    torch.cuda.synchronize()
    assert np.array_equal(S.bits32(dist.cpu().numpy()), S.bits32(got)) and np.array_equal(bits64(scratch), bits64(scratch2))
    # row i = coevo_fc_distance with net i as the reference (whose own distance says NaN, not +0.0, when it holds an inf)
    rows = torch.full((n, n), float("nan"), dtype=torch.float32, device=DEV)
    for i in range(n):
        L.call("coevo_fc_distance", L._p(slab[i]), L._p(slab), n, D, L._p(rows[i]))
    torch.cuda.synchronize()
    rows = rows.cpu().numpy()
    finite = np.isfinite(w[:, gk.linear_mask(D)]).all(axis=1)
    same = S.bits32(rows) == S.bits32(got)
    assert (same | np.diag(~finite)).all() and np.isnan(np.diag(rows)[~finite]).all()


# ------------------------------------------------------------------------------------------------ niche counts
def device_niche(d):
    n = len(d)
    dist = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(DEV)
    out = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    L.call("coevo_niche_counts", L._p(dist), n, L._p(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("D", [8, 10])
def test_niche_counts_of_the_computed_matrices(D):
    for n in S.PAIRWISE_N:
        w, _ = S.crafted(D, "plain", n)
        dist, _ = run_pairwise(to_slab(w, D), n, D)
        out = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
        L.call("coevo_niche_counts", L._p(dist), n, L._p(out))
        torch.cuda.synchronize()
        assert sc.same_f32(out.cpu().numpy(), S.niche(dist.cpu().numpy())), n
        # ... which is coevo_sharing_score on every row
        score = torch.zeros(1, dtype=torch.float32, device=DEV)
        for i in (0, n - 1):
            L.call("coevo_sharing_score", L._p(dist[i]), n, L._p(score))
            assert sc.same_f32(score.cpu().numpy(), out[i:i + 1].cpu().numpy())
    assert np.isnan(device_niche(np.zeros((1, 1)))).all()    # n = 1: the one distance is the self term, 0 / 0


@pytest.mark.parametrize("kind", S.NICHE_CRAFTED)
def test_niche_counts_of_crafted_matrices(kind):
    d = S.niche_matrix(kind)
    got, want = device_niche(d), S.niche(d)
    assert sc.same_f32(got, want)
    if kind in ("single", "zeros"):
        assert np.isnan(got).all()
    if kind == "one_inf":
        assert np.isnan(got).sum() == 2
    if kind == "n257":
        assert len(got) == 257 and np.isfinite(got).all()


# ------------------------------------------------------------------------------------------------ fitness
@pytest.mark.parametrize("hof", [1, 3, 5])
def test_fitness_with_its_switches(hof):
    pop, first = 131, 7     # more than one block of 128 threads, games that do not start at 0
    g = np.random.Generator(np.random.PCG64(40 + hof))
    plain = np.concatenate([g.random((first, 3)), -g.random((pop * hof, 3)) * 20])
    cancel = np.concatenate([g.random((first, 3)), S.cancellation_rewards(pop, hof)])
    share = (g.random(pop) * 3).astype(np.float32)
    share_dev = torch.from_numpy(share).to(DEV)
    for name, r in (("plain", plain), ("cancellation", cancel)):
        rewards = torch.from_numpy(r).to(DEV)
        for slot in range(3):
            for flags in range(4):
                fit = torch.full((pop,), float("nan"), dtype=torch.float32, device=DEV)
                L.call("coevo_ga_fitness_shared", L._p(rewards), first, pop, hof, hof, slot, flags, L._p(share_dev), L._p(fit))
                want = S.fitness(r, hof, hof, slot, flags, share, game_first=first)[:pop]
                assert sc.same_f32(fit.cpu().numpy(), want), (name, slot, flags)
                if flags == 0:
                    old = torch.full((pop,), float("nan"), dtype=torch.float32, device=DEV)
                    L.call("coevo_ga_fitness", L._p(rewards), first, pop, hof, hof, slot, L._p(share_dev), L._p(old))
                    assert sc.same_f32(old.cpu().numpy(), fit.cpu().numpy()), (name, slot)
        if name == "cancellation" and hof >= 3:   # the table can tell: the other order is other words
            assert (S.bits32(want) != S.bits32(S.fitness_reversed(r[first:], hof, hof, 2, share))).any()


# ------------------------------------------------------------------------------------------------ engine
def make_engine(hof_mean, population_sharing):
    E = S.ENGINE
    hof_flat, pop_flat = S.engine_initial()
    eng = ga.GAEngine(E["pop"], E["hof"], E["elites"], limit_train=E["limit"], limit_eval=E["limit"], rng="device_philox",
                      philox_seed=E["philox_seed"], hof_mean=hof_mean, population_sharing=population_sharing)
    eng.load_initial(pop_flat, hof_flat)
    return eng, pop_flat


@pytest.mark.parametrize("hof_mean,population_sharing", S.MODES)
def test_engine_generations_equal_the_statements(hof_mean, population_sharing):
    E = S.ENGINE
    pop, hof, n_el = E["pop"], E["hof"], E["elites"]
    eng, pop0 = make_engine(hof_mean, population_sharing)
    stale = {r: pop0[r][-1] for r in ROLES}
    per = pop * hof
    sigmas = {r: E["sigma"] for r in ROLES}
    for gen in range(2):
        eng.rollout(gen, with_prev_eval=gen > 0)
        eng.ro.check_status()
        rewards = eng.rewards_host()[:eng.n_main].copy()
        before = {r: eng.download(r, "pop", 0, pop) for r in ROLES}
        hof_before = {r: eng.download(r, "hof", 0, hof) for r in ROLES}
        eng.select()
        torch.cuda.synchronize()
        want = {}
        for ri, r in enumerate(ROLES):
            D = rp.ROLE_D[r]
            # what the equalities below rest on, as properties of the inputs
            assert all(sc.dist_order_proof(stale[r], w, D) for w in before[r])
            stale_dist = S.stale_distances(before[r], stale[r], D)
            assert np.array_equal(S.bits32(eng.dist[r].cpu().numpy()), S.bits32(stale_dist)), (gen, r)
            t = want[r] = S.generation_tail(rewards[ri * per:(ri + 1) * per], before[r], stale_dist, D, ri, gen, hof, n_el,
                                            E["sigma"], E["philox_seed"], hof_mean, population_sharing)
            if population_sharing:
                assert S.pairwise_order_proof(before[r], D) and S.niche_order_proof(t["pair_dist"])
                assert np.array_equal(S.bits32(eng.pair_dist[r].cpu().numpy()), S.bits32(t["pair_dist"])), (gen, r)
                assert sc.same_f32(eng.niche[r].cpu().numpy(), t["niche"]), (gen, r)
            else:
                assert S.niche_order_proof([stale_dist])
                assert sc.same_f32(eng.div[r].cpu().numpy(), t["diversity"]), (gen, r)
            assert np.array_equal(S.bits32(eng.fitness[r].cpu().numpy()), S.bits32(t["fitness"])), (gen, r)
            assert eng.order[r].cpu().numpy().tolist() == t["order"] and eng.elite_ids()[r] == t["elite_ids"], (gen, r)
            assert S.bits32(eng.best_dist[r].cpu().numpy()).ravel()[0] == S.bits32(t["best_dist"]).ravel()[0], (gen, r)
        eng.breed_device(gen, sigmas)
        for ri, r in enumerate(ROLES):
            t = want[r]
            after = eng.download(r, "pop", 0, pop)
            assert np.array_equal(S.bits32(after[0]), S.bits32(before[r][t["order"][0]])), (gen, r)
            assert np.array_equal(S.bits32(after[1:]), S.bits32(np.stack(t["children"]))), (gen, r)
            # the Hall of Fame moved FIFO: the oldest out, the best in at the end
            hof_after = eng.download(r, "hof", 0, hof)
            assert np.array_equal(S.bits32(hof_after[:-1]), S.bits32(hof_before[r][1:])), (gen, r)
            assert np.array_equal(S.bits32(hof_after[-1]), S.bits32(before[r][t["order"][0]])), (gen, r)
            assert np.array_equal(S.bits32(eng.download(r, "elite", 0, n_el)),
                                  S.bits32(before[r][t["elite_ids"]])), (gen, r)


def test_engine_with_the_modes_off_gives_coevo_ga_selects_words(monkeypatch):
    E = S.ENGINE
    pop, hof = E["pop"], E["hof"]
    eng, _ = make_engine(False, False)
    assert not hasattr(eng, "niche") and not hasattr(eng, "pair_dist")
    calls = []
    real = L.call
    with monkeypatch.context() as m:
        m.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        eng.rollout(0, with_prev_eval=False)
        eng.select()
    torch.cuda.synchronize()
    assert "coevo_ga_select" in calls and not [c for c in calls if c in L.sharing_symbols()]
    rewards = torch.from_numpy(eng.rewards_host().copy()).to(DEV)
    per = pop * hof
    for ri, r in enumerate(ROLES):
        fit = torch.full((pop,), float("nan"), dtype=torch.float32, device=DEV)
        L.call("coevo_ga_fitness_shared", L._p(rewards), ri * per, pop, hof, hof, ri, 0, L._p(eng.div[r]), L._p(fit))
        assert np.array_equal(S.bits32(fit.cpu().numpy()), S.bits32(eng.fitness[r].cpu().numpy()))
        want = S.fitness(eng.rewards_host()[ri * per:(ri + 1) * per], hof, hof, ri, 0, eng.div[r].cpu().numpy())
        assert np.array_equal(S.bits32(want), S.bits32(eng.fitness[r].cpu().numpy()))
        assert eng.order[r].cpu().numpy().tolist() == gk.rank_desc(want)


# ------------------------------------------------------------------------------------------------ trainer
def test_trainer_with_both_switches_equals_the_engine_driven_by_hand(tmp_path):
    cfg = dict(generations=3, population=8, hof_size=3, elites_number=2, max_timesteps_per_episode=9, max_evaluation_steps=9,
               adaptive=False, coevo_hof_mean=True, coevo_population_sharing=True)
    torch.manual_seed(11)
    args = Bag(algorithm="GA", **cfg)
    env = initialize_env(args)
    res = ga.genetic_algorithm_train(env, env.agents[0], args, str(tmp_path), rng="device_philox")
    tr_eng = res.engine
    assert tr_eng.hof_mean and tr_eng.population_sharing
    # the same engine by hand
    torch.manual_seed(11)
    args2 = Bag(algorithm="GA", **cfg)
    env2 = initialize_env(args2)
    pop_flat, hof_flat = ga.initial_population(env2, args2)
    eng = ga.GAEngine(8, 3, 2, limit_train=9, limit_eval=9, rng="device_philox", first_ordinal=getattr(env2, "n_resets", 1),
                      env_seed=getattr(env2, "seed_value", ga.ENV_SEED) or ga.ENV_SEED, hof_mean=True, population_sharing=True)
    eng.load_initial(pop_flat, hof_flat)
    sigmas = {r: 0.05 for r in ROLES}
    for gen in range(3):
        eng.rollout(gen, with_prev_eval=gen > 0)
        eng.ro.check_status()
        eng.select()
        assert np.array_equal(eng.rewards_host()[:eng.n_main], res.game_rewards[gen])
        assert [eng.fitness[r].cpu().numpy().tolist() for r in ROLES] == res.fitness[gen]
        assert [eng.elite_ids()[r] for r in ROLES] == res.elite_ids[gen]
        mean_niche = [float(np.mean(eng.niche[r].cpu().numpy().astype(np.float64))) for r in ROLES]
        assert res.diversity[gen] == mean_niche and all(np.isfinite(mean_niche)) and min(mean_niche) >= 1.0
        eng.breed_device(gen, sigmas)
    for r in ROLES:
        for region, n in (("pop", 8), ("hof", 3), ("elite", 2)):
            assert np.array_equal(S.bits32(eng.download(r, region, 0, n)), S.bits32(tr_eng.download(r, region, 0, n))), (r, region)
        assert np.array_equal(S.bits32(eng.niche[r].cpu().numpy()), S.bits32(tr_eng.niche[r].cpu().numpy()))
    lines = [json.loads(x) for x in open(os.path.join(tmp_path, "metrics.jsonl"))]
    assert len(lines) == 3 and [ln["diversity"] for ln in lines] == res.diversity
