"""The float16 breeding of several roles in one launch (coevo_fc16_perturb_dist_multi, coevo_fc16_distance_finalize_multi) on
the GPU, equalities only: every word a mixed launch writes - children, distance partials, distances, the head word - against
the per-job calls (coevo_fc16_perturb_dist, coevo_fc16_distance_finalize; those are pinned to the CPU checker by
tests/test_fp16_breeding_gpu.py), the refusals, and whole generations of the half engines with ``multi_breed=True`` against
the default engines."""
import ctypes as ct

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.es_half import HalfESEngine
from coevonet_amd.ga_half import HalfGAEngine
from oracle import ref_port as rp
from tests import ga16_checker as gk
from tests.test_fp16_gpu import random_flat
from tests.util import sha

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7fc07e00   # NaN as an fp32 word and in both of its halves
GUARD64 = 0x7ff8dead0000beef   # a NaN double no sum produces
SEED = 0x1234567890abcdef
STREAM_LO, STREAM_HI, GEN = 5, 9, 3
N_GUARD = 8


def pack16(flats, D):
    flats = np.ascontiguousarray(np.stack(flats), dtype=np.float32)
    slab = torch.full((len(flats) * L.fc16_slab_stride(D),), POISON, dtype=torch.int32, device=DEV)
    L.call("coevo_fc16_pack", L._p(torch.from_numpy(flats).to(DEV)), L._p(slab), len(flats), D)
    return slab


def guarded_f64(n):
    return torch.from_numpy(np.full(n + N_GUARD, GUARD64, dtype=np.uint64).view(np.int64)).to(DEV).view(torch.float64)


def words64(t):
    return t.view(torch.int64).cpu().numpy().view(np.uint64)


# (D, child_first, n_children, nets in the child slab, sigma, with distance): an empty job sits between the others
JOBS = ((10, 1, 3, 5, 0.0, True), (10, 2, 1, 4, 0.5, False), (10, 0, 0, 2, 0.1, True), (8, 0, 2, 3, 0.005, True))


class Fixture:
    """parents, reference nets and sigmas of JOBS (shared), and one set of poisoned outputs"""

    def __init__(self, jobs=JOBS):
        rng = np.random.default_rng(77)
        self.jobs = jobs
        self.par = [pack16([random_flat(rng, D), random_flat(rng, D, scale=0.15)], D) for D, *_ in jobs]
        self.ref = [pack16([random_flat(rng, D)], D) for D, *_ in jobs]
        self.idx = torch.tensor([c % 2 for c in range(4)], dtype=torch.int32, device=DEV)
        self.sig = [torch.tensor([s], dtype=torch.float32, device=DEV) for *_, s, _ in jobs]
        self.gen = torch.tensor([GEN], dtype=torch.int32, device=DEV)

    def outputs(self):
        child = [torch.full((nets * L.fc16_slab_stride(D),), POISON, dtype=torch.int32, device=DEV)
                 for D, _, _, nets, _, _ in self.jobs]
        part = [guarded_f64(n * L.fc16_perturb_blocks(D)) if dist else None for D, _, n, _, _, dist in self.jobs]
        return child, part

    def job(self, j, child, part):
        D, first, n, _, _, dist = self.jobs[j]
        return L.Perturb16Job(L._p(self.par[j]), L._p(self.idx), L._p(child[j]), L._p(self.sig[j]),
                              L._p(self.ref[j]) if dist else None, L._p(part[j]) if dist else None, first, n, D, STREAM_LO,
                              STREAM_HI, 0)

    def per_job(self, flags):
        """the per-job calls with the generation folded into stream_hi on the host"""
        child, part = self.outputs()
        for j, (D, first, n, _, _, dist) in enumerate(self.jobs):
            L.call("coevo_fc16_perturb_dist", L._p(self.par[j]), L._p(self.idx), L._p(child[j]), first, n, D, L._p(self.sig[j]),
                   SEED, STREAM_LO, STREAM_HI + 4 * GEN, flags, None, L._p(self.ref[j]) if dist else None,
                   L._p(part[j]) if dist else None)
        torch.cuda.synchronize()
        return child, part

    def multi(self, flags, which=None):
        """one launch over the jobs `which` (default: all), the generation read from the device"""
        which = list(range(len(self.jobs))) if which is None else which
        child, part = self.outputs()
        arr = (L.Perturb16Job * len(which))(*[self.job(j, child, part) for j in which])
        L.call("coevo_fc16_perturb_dist_multi", ct.cast(arr, ct.c_void_p), len(which), SEED, flags, L._p(self.gen))
        torch.cuda.synchronize()
        return child, part


def assert_same_outputs(fx, got, want, which=None):
    which = list(range(len(fx.jobs))) if which is None else which
    for j, (D, first, n, nets, _, dist) in enumerate(fx.jobs):
        stride = L.fc16_slab_stride(D)
        g = got[0][j].cpu().numpy().view(np.uint32).reshape(nets, stride)
        w = want[0][j].cpu().numpy().view(np.uint32).reshape(nets, stride)
        written = range(first, first + n) if j in which else range(0)
        for net in range(nets):
            if net in written:
                assert np.array_equal(g[net], w[net]), (j, net, "child differs from the per-job call's")
                assert (g[net] != POISON).any()
            else:
                assert (g[net] == POISON).all(), (j, net, "a neighbour of the written nets changed")
        if dist:
            gp, wp = words64(got[1][j]), words64(want[1][j])
            nb = L.fc16_perturb_blocks(D)
            assert (gp[n * nb:] == GUARD64).all() and len(gp) == n * nb + N_GUARD, (j, "guard words behind the partials")
            if j in which:
                assert np.array_equal(gp, wp), (j, "partials differ from the per-job call's")
                assert (gp[:n * nb] != GUARD64).all(), (j, "a partial was not written")
            else:
                assert (gp == GUARD64).all()


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.mark.parametrize("flags", [0, 1])
def test_mixed_jobs_in_one_launch_equal_the_per_job_calls(fx, flags):
    assert (L.fc16_perturb_blocks(10), L.fc16_perturb_blocks(8)) == (70, 69)
    want = fx.per_job(flags)
    got = fx.multi(flags)
    assert_same_outputs(fx, got, want)
    assert int(fx.gen.item()) == GEN
    # the D = 8 job's partials at stride 69 beside the D = 10 job's at stride 70: child c's sums start at c * stride, each
    # buffer ends in its guard words (assert_same_outputs); fc2.weight alone fills 64 blocks of every child, whose sums are
    # positive (a block of LayerNorm entries or padding sums to 0)
    for j, nb in ((0, 70), (3, 69)):
        n = JOBS[j][2]
        p = got[1][j].cpu().numpy()[:n * nb].reshape(n, nb)
        assert np.isfinite(p).all() and ((p > 0).sum(axis=1) >= 64).all(), j
    # sigma 0: the children are their parents' words
    stride = L.fc16_slab_stride(10)
    c0 = got[0][0].cpu().numpy().view(np.uint32).reshape(5, stride)
    p0 = fx.par[0].cpu().numpy().view(np.uint32).reshape(2, stride)
    for c in range(3):
        assert np.array_equal(c0[1 + c], p0[c % 2])
    if flags:   # LayerNorm left alone at sigma 0.5: the child's LayerNorm entries are its parent's
        child = torch.zeros(1, L.fc_param_count(10), dtype=torch.float32, device=DEV)
        parent = torch.zeros(1, L.fc_param_count(10), dtype=torch.float32, device=DEV)
        L.call("coevo_fc16_unpack", got[0][1].data_ptr() + 4 * 2 * stride, L._p(child), 1, 10)
        L.call("coevo_fc16_unpack", L._p(fx.par[1]), L._p(parent), 1, 10)
        m = gk.linear_mask(10)
        child, parent = child.cpu().numpy()[0], parent.cpu().numpy()[0]
        assert np.array_equal(child[~m].view(np.uint32), parent[~m].view(np.uint32)) and (child[m] != parent[m]).mean() > 0.9


@pytest.mark.parametrize("which", [[0], [3], [1], [3, 0], [2]])
def test_one_and_two_jobs(fx, which):
    """n_jobs 1 (a D = 10 job, the D = 8 job, a job without a distance, an empty job: no launch) and the narrow job first"""
    want = fx.per_job(0)
    got = fx.multi(0, which)
    assert_same_outputs(fx, got, want, which)


def finalize_case(rng):
    """(partials, n_blocks, n, first, head or None, length of dist) per job: a head with first 1, no head with first 0, no
    head with first 2, an empty job"""
    out = []
    for n_blocks, n, first, head, length in ((70, 3, 1, np.float32(np.float16(3.14159)), 6), (69, 2, 0, None, 4),
                                             (5, 4, 2, None, 8), (70, 0, 1, np.float32(1.5), 3)):
        part = torch.from_numpy(rng.random(max(n, 1) * n_blocks) * 100).to(DEV)
        out.append((part, n_blocks, n, first, None if head is None else torch.tensor([head], dtype=torch.float32, device=DEV),
                    length))
    return out


@pytest.mark.parametrize("n_jobs", [1, 3, 4])
def test_multi_finalize_equals_the_single_finalizes(n_jobs):
    cases = finalize_case(np.random.default_rng(5))[:n_jobs]
    nan = lambda k: torch.full((k,), float("nan"), dtype=torch.float32, device=DEV)   # noqa: E731
    want, got = [nan(c[5]) for c in cases], [nan(c[5]) for c in cases]
    jobs = (L.FinalizeJob * n_jobs)()
    for j, (part, n_blocks, n, first, head, _) in enumerate(cases):
        if n > 0:   # (the single call refuses n == 0; the multi launch skips such a job)
            L.call("coevo_fc16_distance_finalize", L._p(part), n_blocks, n, L._p(want[j]), first, L._p(head))
        jobs[j] = L.FinalizeJob(L._p(part), L._p(got[j]), L._p(head), n_blocks, n, first, 0)
    L.call("coevo_fc16_distance_finalize_multi", ct.cast(jobs, ct.c_void_p), n_jobs)
    torch.cuda.synchronize()
    for j, (part, n_blocks, n, first, head, length) in enumerate(cases):
        g, w = got[j].cpu().numpy(), want[j].cpu().numpy()
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), j
        written = set(range(first, first + n)) | ({first - 1} if head is not None and n > 0 else set())
        assert [i for i in range(length) if not np.isnan(g[i])] == sorted(written), (j, "words outside the job's range")
        if n > 0:
            assert (g[first:first + n] == g[first:first + n].astype(np.float16)).all() and (g[first:first + n] > 0).all()
            if head is not None:
                assert g[first - 1] == head.item()


def test_bad_arguments_return_err_arg_and_write_nothing(fx):
    lib, st = L.load(), L._stream()
    child, part = fx.outputs()
    good = [fx.job(j, child, part) for j in range(4)]

    def perturb(jobs, n=None, flags=0):
        arr = (L.Perturb16Job * max(len(jobs), 1))(*jobs)
        return lib.coevo_fc16_perturb_dist_multi(ct.cast(arr, ct.c_void_p), len(jobs) if n is None else n, SEED, flags, None, st)

    def with_(j, **kw):
        jobs = [L.Perturb16Job.from_buffer_copy(g) for g in good]
        for k, v in kw.items():
            setattr(jobs[j], k, v)
        return jobs

    assert lib.coevo_fc16_perturb_dist_multi(None, 1, SEED, 0, None, st) == -1
    assert perturb(good, n=0) == -1 and perturb(good + good[:1], n=5) == -1 and perturb(good, n=-1) == -1
    for flags in (2, 3, -1, 4):
        assert perturb(good, flags=flags) == -1, flags
    bad = [dict(parent_slab=None), dict(parent_idx=None), dict(child_slab=None), dict(sigma_dev=None), dict(D=9), dict(D=0),
           dict(n_children=-1), dict(n_children=65536), dict(child_first=-1), dict(dist_ref=None), dict(dist_partial=None),
           dict(parent_slab=good[0].parent_slab + 4), dict(child_slab=good[0].child_slab + 8), dict(dist_ref=good[0].dist_ref + 4)]
    for kw in bad:
        assert perturb(with_(0, **kw)) == -1, kw
    assert perturb(with_(3, D=12)) == -1, "a bad job behind good ones: nothing of the good ones is launched"
    assert perturb(with_(2, parent_slab=None)) == -1, "an empty job is checked like any other"
    assert perturb(with_(1, dist_ref=good[0].dist_ref)) == -1, "exactly one of dist_ref / dist_partial"
    # all jobs empty: OK, and no launch
    assert perturb([good[2]]) == 0 and perturb([good[2], good[2]]) == 0
    # the finalize
    dist = torch.full((6,), float("nan"), dtype=torch.float32, device=DEV)
    p = torch.ones(3 * 70, dtype=torch.float64, device=DEV)
    ok = L.FinalizeJob(L._p(p), L._p(dist), L._p(dist), 70, 3, 1, 0)

    def finalize(n=None, **kw):
        arr = (L.FinalizeJob * 5)(*[L.FinalizeJob.from_buffer_copy(ok) for _ in range(5)])
        for k, v in kw.items():
            setattr(arr[1], k, v)
        return lib.coevo_fc16_distance_finalize_multi(ct.cast(arr, ct.c_void_p), 2 if n is None else n, st)

    assert lib.coevo_fc16_distance_finalize_multi(None, 1, st) == -1
    assert finalize(n=0) == -1 and finalize(n=5) == -1
    for kw in (dict(dist_partial=None), dict(dist=None), dict(n_blocks=0), dict(n=-1), dict(first=-1), dict(first=0)):
        assert finalize(**kw) == -1, kw   # (first 0 with a head: the head word would lie in front of the array)
    empty = (L.FinalizeJob * 1)(L.FinalizeJob(L._p(p), L._p(dist), None, 70, 0, 0, 0))
    assert lib.coevo_fc16_distance_finalize_multi(ct.cast(empty, ct.c_void_p), 1, st) == 0
    torch.cuda.synchronize()
    for c in child:
        assert (c.cpu().numpy().view(np.uint32) == POISON).all()
    for q in part:
        assert q is None or (words64(q) == GUARD64).all()
    assert torch.isnan(dist).all()
    for j, s in enumerate(fx.sig):
        assert float(s.item()) == np.float32(JOBS[j][4])


# ---------------------------------------------------------------------------------------------- whole generations
SIGMAS = {"agent_0": 0.05, "agent_1": 0.02, "adversary_0": 0.1}
GENERATIONS = 2


def eq64(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_two_ga_generations_with_multi_breed_equal_the_default_engine():
    torch.manual_seed(3)
    hof, popu = rp.ga_initial(4, 2)
    rnd = lambda d: {r: np.stack([gk.round_linear(w, gk.ROLE_D[r]) for w in d[r]]) for r in gk.ROLES}   # noqa: E731
    pop_flat, hof_flat = rnd(popu), rnd(hof)
    runs = []
    for multi in (False, True):
        eng = HalfGAEngine(4, 2, 2, 6, 6, philox_seed=11, multi_breed=multi)
        eng.load_initial(pop_flat, hof_flat)
        rec = []
        for gen in range(GENERATIONS):
            eng.rollout(gen)
            rewards = eng.rewards_host().copy()
            eng.select()
            eng.breed(gen, SIGMAS)
            torch.cuda.synchronize()
            rec.append(dict(rewards=rewards, ids=eng.elite_ids(), dist={r: eng.dist[r].cpu().numpy() for r in gk.ROLES},
                            nets={(r, region): [sha(w) for w in eng.download(r, region, 0, n)] for r in gk.ROLES
                                  for region, n in (("pop", 4), ("hof", 2), ("elite", 2))}))
        rec.append(dict(ev=eng.eval_only(GENERATIONS - 1), rewards=eng.rewards_host().copy()))
        runs.append((rec, eng.slab.cpu().numpy()))
    (plain, slab0), (multi, slab1) = runs
    for gen in range(GENERATIONS):
        assert eq64(plain[gen]["rewards"], multi[gen]["rewards"]), (gen, "reward triples")
        assert plain[gen]["ids"] == multi[gen]["ids"]
        for r in gk.ROLES:
            assert np.array_equal(bits(plain[gen]["dist"][r]), bits(multi[gen]["dist"][r])), (gen, r, "distances")
            assert not np.isnan(multi[gen]["dist"][r]).any()
        assert plain[gen]["nets"] == multi[gen]["nets"], (gen, "nets")
    assert plain[-1]["ev"] == multi[-1]["ev"] and eq64(plain[-1]["rewards"], multi[-1]["rewards"])
    assert np.array_equal(slab0, slab1)
    assert plain[0]["nets"] != plain[1]["nets"], "breeding must move the population"


def test_two_es_generations_with_multi_breed_equal_the_default_engine():
    torch.manual_seed(3)
    base = {r: gk.round_linear(rp.init_net(gk.ROLE_D[r]), gk.ROLE_D[r]) for r in gk.ROLES}
    runs = []
    for multi in (False, True):
        eng = HalfESEngine(6, 6, 6, philox_seed=11, multi_breed=multi)
        keep = [eng.upload(r, "base", 0, base[r][None]) for r in gk.ROLES]
        torch.cuda.current_stream().synchronize()
        del keep
        rec = []
        for gen in range(GENERATIONS):
            eng.perturb(gen, SIGMAS, True)
            pert = {r: [sha(w) for w in eng.download(r, "pert", 0, 6)] for r in gk.ROLES}
            eng.rollout(gen)
            eng.update(gen, 0.1, True)
            ev = eng.evaluate(gen)
            rec.append(dict(pert=pert, rewards=eng.rewards_host().copy(), ev=ev, eval_games=eng.eval_ro.rewards.cpu().numpy(),
                            dist={r: eng.dist[r].cpu().numpy() for r in gk.ROLES},
                            fit={r: eng.fitness[r].cpu().numpy() for r in gk.ROLES}, div=eng.diversity(),
                            base={r: sha(eng.download(r, "base", 0, 1)[0]) for r in gk.ROLES}))
        runs.append((rec, eng.slab.cpu().numpy()))
    (plain, slab0), (multi, slab1) = runs
    for gen in range(GENERATIONS):
        a, b = plain[gen], multi[gen]
        assert a["pert"] == b["pert"] and a["base"] == b["base"], (gen, "nets")
        assert eq64(a["rewards"], b["rewards"]) and eq64(a["eval_games"], b["eval_games"]) and a["ev"] == b["ev"], gen
        for r in gk.ROLES:
            assert np.array_equal(bits(a["dist"][r]), bits(b["dist"][r])) and (b["dist"][r] > 0).all(), (gen, r, "distances")
            assert np.array_equal(bits(a["fit"][r]), bits(b["fit"][r])), (gen, r, "fit16")
            assert bits(a["div"][r]) == bits(b["div"][r]), (gen, r, "sharing score")
    assert np.array_equal(slab0, slab1)
    assert plain[0]["base"] != plain[1]["base"], "the update must move the base nets"
