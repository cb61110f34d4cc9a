"""The float16 Co-GA extension modes on the MI355X: coevo_fc16_pairwise_distance (include/coevo_sharing16.h) against the numpy
statement of tests/sharing16_cases.py and against coevo_fc16_distance + coevo_fc16_distance_finalize row by row, the niche
counts of its matrices, and HalfGAEngine under the three non-default mode pairs against the CPU checker - all bit equalities
(the inputs are order-proof: see tests/sharing_cases.py)."""
import functools
import hashlib

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.ga_half import HalfGAEngine
from oracle import ref_port as rp
from tests import ga16_checker as gk
from tests import select_cases as sc
from tests import sharing16_cases as S16
from tests import sharing_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROLES = rp.ROLES
NAN32 = 0x7FC00000


def used_words(D):
    """words of an fp16 slab net before the stride's padding (fc16_layout.hip.h f16_used)"""
    return 256 * 256 + D * 256 + 5 * 128 + 3 * 512 + 3 * 256 + 5


def to_slab16(flats, D):
    """flat parameters() vectors of fp16 values -> a device fp16 slab [n][stride] whose padding words are NaN"""
    n, stride = len(flats), L.fc16_slab_stride(D)
    slab = torch.full((n, stride), NAN32, dtype=torch.int32, device=DEV)
    flat = torch.from_numpy(np.ascontiguousarray(flats, dtype=np.float32)).to(DEV)
    L.call("coevo_fc16_pack", L._p(flat), L._p(slab), n, D)
    assert stride > used_words(D)
    slab[:, used_words(D):] = NAN32
    torch.cuda.synchronize()
    return slab


def run_pairwise16(slab, n, D, scratch=None, dist=None):
    """scratch poisoned with NaN and dist pre-filled with NaN unless given"""
    if scratch is None:
        scratch = torch.full((int(L.load().coevo_fc16_pairwise_scratch_doubles(n, D)),), float("nan"), dtype=torch.float64,
                             device=DEV)
    if dist is None:
        dist = torch.full((n, n), float("nan"), dtype=torch.float32, device=DEV)
    L.call("coevo_fc16_pairwise_distance", L._p(slab), n, D, L._p(scratch), L._p(dist))
    torch.cuda.synchronize()
    return dist, scratch


def rows_by_distance(slab, n, D):
    """row i = coevo_fc16_distance of every net to net i + coevo_fc16_distance_finalize"""
    nb = L.fc16_perturb_blocks(D)
    part = torch.full((n * nb,), float("nan"), dtype=torch.float64, device=DEV)
    rows = torch.full((n, n), float("nan"), dtype=torch.float32, device=DEV)
    for i in range(n):
        L.call("coevo_fc16_distance", L._p(slab[i]), L._p(slab), n, D, L._p(part))
        L.call("coevo_fc16_distance_finalize", L._p(part), nb, n, L._p(rows[i]), 0, None)
    torch.cuda.synchronize()
    return rows.cpu().numpy()


# ------------------------------------------------------------------------------------------------ pairwise distances
PAIRWISE_CASES = [("plain", n) for n in S.PAIRWISE_N] + [(k, n) for k in S16.CRAFTED for n in S16.CRAFTED_N]


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("kind,n", PAIRWISE_CASES)
def test_pairwise_distances(D, kind, n):
    w, want = S16.crafted(D, kind, n)
    slab = to_slab16(w, D)
    dist, scratch = run_pairwise16(slab, n, D)
    got = dist.cpu().numpy()
    assert np.array_equal(S.bits32(got), S.bits32(want))                      # the numpy statement, every word written
    assert np.array_equal(S.bits32(got), S.bits32(got.T)) and not S.bits32(np.diag(got)).any()
    if kind == "identical":
        assert S.bits32(got[0, n - 1]) == 0
    if kind == "inf":
        k = n // 2
        assert np.isposinf(np.delete(got[k], k)).all() and np.isposinf(np.delete(got[:, k], k)).all()
    if kind == "extreme":
        assert np.isposinf(got[0, n - 1]) and np.isfinite(got).sum() == n * n - 2
    if kind == "subnormal":
        assert got[0, n - 1] == np.float32(21 * 2.0 ** -24)
    if kind == "rounding":
        assert got[0, n - 1] == S16.ROUNDING_CONTRACT != S16.ROUNDING_UNROUNDED
    # a second run on the used scratch and output: the same words
    dist2, scratch2 = run_pairwise16(slab, n, D, scratch, dist)
    assert np.array_equal(S.bits32(dist2.cpu().numpy()), S.bits32(got))
    # row i = coevo_fc16_distance with net i as the reference (whose own distance says NaN, not +0.0, when it holds an inf)
    rows = rows_by_distance(slab, n, D)
    finite = np.isfinite(w[:, gk.linear_mask(D)]).all(axis=1)
    same = S.bits32(rows) == S.bits32(got)
    assert (same | np.diag(~finite)).all() and np.isnan(np.diag(rows)[~finite]).all()


# ------------------------------------------------------------------------------------------------ niche counts
@pytest.mark.parametrize("D", [8, 10])
def test_niche_counts_of_the_fp16_matrices(D):
    for n in S.PAIRWISE_N:
        w, want = S16.crafted(D, "plain", n)
        dist, _ = run_pairwise16(to_slab16(w, D), n, D)
        out = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
        L.call("coevo_niche_counts", L._p(dist), n, L._p(out))
        torch.cuda.synchronize()
        assert np.array_equal(S.bits32(dist.cpu().numpy()), S.bits32(want))
        assert sc.same_f32(out.cpu().numpy(), S.niche(want)), n


# ------------------------------------------------------------------------------------------------ engine
E = S.ENGINE
SIGMAS = {r: E["sigma"] for r in ROLES}
GENERATIONS = 2


def sha(w):
    return hashlib.sha256(np.ascontiguousarray(w, dtype=np.float32).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def checker_run(hof_mean, population_sharing):
    """the checker's two generations under the modes, computed once: per generation the record and the nets after it"""
    hof, pop = S16.engine_initial()
    st = gk.State(pop, hof)
    out = []
    for gen in range(GENERATIONS):
        rec = S16.generation(st, gen, E["sigma"], E["elites"], E["limit"], E["philox_seed"], hof_mean, population_sharing)
        rec["nets"] = {(r, region): [sha(w) for w in nets[r]] for r in ROLES
                       for region, nets in (("pop", st.popu), ("hof", st.hof), ("elite", st.elites))}
        out.append(rec)
    return out


def make_engine(**kw):
    eng = HalfGAEngine(E["pop"], E["hof"], E["elites"], E["limit"], E["limit"], philox_seed=E["philox_seed"], **kw)
    hof, pop = S16.engine_initial()
    eng.load_initial(pop, hof)
    return eng


def engine_nets(eng):
    counts = {"pop": eng.pop, "hof": eng.hof, "elite": eng.E}
    return {(r, region): [sha(w) for w in eng.download(r, region, 0, n)] for r in ROLES for region, n in counts.items()}


def drive(eng):
    """two generations by hand -> per generation {rewards, fitness, niche / div, order, pair_dist, dist, nets}"""
    out = []
    for gen in range(GENERATIONS):
        eng.rollout(gen)
        rew = eng.rewards_host().copy()
        eng.select()
        torch.cuda.synchronize()
        rec = {"rewards": rew, "dist": {r: eng.dist[r].cpu().numpy().copy() for r in ROLES},
               "fitness": {r: eng.fitness[r].cpu().numpy().copy() for r in ROLES}, "elite_ids": eng.elite_ids(),
               "order": {r: eng.order[r].cpu().numpy().tolist() for r in ROLES},
               "best_dist": {r: eng.best_dist[r].cpu().numpy().copy() for r in ROLES}}
        if eng.population_sharing:
            rec["niche"] = {r: eng.niche[r].cpu().numpy().copy() for r in ROLES}
            rec["pair_dist"] = {r: eng.pair_dist[r].cpu().numpy().copy() for r in ROLES}
        else:
            rec["div"] = {r: eng.div[r].cpu().numpy().copy() for r in ROLES}
        eng.breed(gen, SIGMAS)
        rec["nets"] = engine_nets(eng)
        out.append(rec)
    eng.eval_only(GENERATIONS - 1)
    out.append(eng.rewards_host()[eng.n_main:].copy())
    return out


def eq64(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("hof_mean,population_sharing", S.MODES)
def test_engine_generations_against_the_checker(hof_mean, population_sharing):
    want = checker_run(hof_mean, population_sharing)
    eng = make_engine(hof_mean=hof_mean, population_sharing=population_sharing)
    got = drive(eng)
    per = E["pop"] * E["hof"]
    for gen, (g, w) in enumerate(zip(got, want)):
        assert eq64(g["rewards"][:eng.n_main], w["games"]), (gen, "main games")
        if gen > 0:
            assert eq64(g["rewards"][eng.n_main:], want[gen - 1]["eval_games"]), (gen, "evaluation games")
        for ri, r in enumerate(ROLES):
            t = w["tails"][r]
            assert len(set(t["fitness"].tolist())) == E["pop"], (gen, r, "choose inputs whose fitnesses do not tie")
            assert np.array_equal(S.bits32(g["dist"][r]), S.bits32(t["stale_dist"])), (gen, r)
            assert np.array_equal(S.bits32(g["fitness"][r]), S.bits32(t["fitness"])), (gen, r)
            assert g["order"][r] == t["order"] and g["elite_ids"][r] == t["elite_ids"], (gen, r)
            assert S.bits32(g["best_dist"][r])[0] == S.bits32(t["best_dist"]), (gen, r)
            if population_sharing:
                assert np.array_equal(S.bits32(g["pair_dist"][r]), S.bits32(t["pair_dist"])), (gen, r)
                assert sc.same_f32(g["niche"][r], t["niche"]), (gen, r)
            else:
                assert sc.same_f32(g["div"][r], t["diversity"]), (gen, r)
            assert eq64(g["rewards"][ri * per:(ri + 1) * per], w["games"][ri * per:(ri + 1) * per])
        assert g["nets"] == w["nets"], (gen, "nets after breeding")
    assert eq64(got[-1], want[-1]["eval_games"])
    # run(): the same elites; under population_sharing the mean niche counts are its diversity
    res = make_engine(hof_mean=hof_mean, population_sharing=population_sharing).run(GENERATIONS, SIGMAS)
    assert res["elite_ids"] == [g["elite_ids"] for g in got[:GENERATIONS]]
    if population_sharing:
        assert res["diversity"] == [{r: float(np.mean(g["niche"][r].astype(np.float64))) for r in ROLES}
                                    for g in got[:GENERATIONS]]


def _same_records(a, b):
    for x, y in zip(a[:GENERATIONS], b[:GENERATIONS]):
        assert eq64(x["rewards"], y["rewards"]) and x["nets"] == y["nets"] and x["order"] == y["order"]
        for key in ("dist", "fitness", "best_dist", "niche", "pair_dist", "div"):
            if key in x or key in y:
                assert all(np.array_equal(S.bits32(x[key][r]), S.bits32(y[key][r])) for r in ROLES), key
    assert eq64(a[-1], b[-1])


def test_multi_breed_gives_the_same_generations_with_the_modes_on():
    modes = dict(hof_mean=True, population_sharing=True)
    plain, multi = make_engine(**modes), make_engine(multi_breed=True, **modes)
    _same_records(drive(plain), drive(multi))
    assert np.array_equal(plain.slab.cpu().numpy(), multi.slab.cpu().numpy())


def test_the_modes_off_give_the_default_engine():
    default, off = make_engine(), make_engine(hof_mean=False, population_sharing=False)
    assert not hasattr(off, "niche") and not hasattr(off, "pair_dist")
    _same_records(drive(default), drive(off))
    assert np.array_equal(default.slab.cpu().numpy(), off.slab.cpu().numpy())
