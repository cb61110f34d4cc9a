"""The float16 trainers without a GPU: every refusal of GATrainer / ESTrainer / genetic_algorithm_train /
evolution_strategy_train before the library is loaded, and the launch scripts of the half engines - default construction names
no ``_multi`` entry, ``multi_breed=True`` replaces the per-role child / distance calls by one multi launch each whose jobs
carry the per-role calls' arguments.  (The two multi-launch symbols in the header and the binding and the job mirror's layout:
tests/test_abi.py.)"""
import types

import pytest

from coevonet_amd import lib as L
from tests.golden import make_golden_launches as mg

NEW =("coevo_fc16_perturb_dist_multi", "coevo_fc16_distance_finalize_multi")
JOB_ARRAYS = {"coevo_fc16_perturb_dist_multi": "Perturb16Job", "coevo_fc16_distance_finalize_multi": "FinalizeJob"}


class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------------------ refusals
GA_MSG, ES_MSG = "Co-GA training with precision float16", "Co-ES with precision float16"


def _ga_calls(args, **kw):
    from coevonet_amd import genetic_algorithm as ga
    return (lambda: ga.GATrainer(None, args, **kw), lambda: ga.genetic_algorithm_train(None, None, args, None, **kw))


def _es_calls(args, **kw):
    from coevonet_amd import evolutionary_strategy as es
    return (lambda: es.ESTrainer(None, args, **kw), lambda: es.evolution_strategy_train(None, args, None, **kw))


def test_every_refusal_comes_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    rank1 = types.SimpleNamespace(rank=1, world=2, gather_ga=lambda eng: None, gather_es=lambda eng, what: None)
    rank0 = types.SimpleNamespace(rank=0, world=2, gather_ga=lambda eng: None, gather_es=lambda eng, what: None)
    for calls, msg in ((_ga_calls, GA_MSG), (_es_calls, ES_MSG)):
        half = lambda **kw: Bag(precision="float16", **kw)   # noqa: E731 - nothing else: no other attribute may be read first
        cases = [
            (half(), {}),                                                       # the default rng, host_reference
            (half(), dict(rng="host_reference")),
            (half(coevo_rng="host_reference"), {}),
            (half(coevo_rng="device_philox"), dict(rng="host_reference")),      # the argument wins
            (half(), dict(rng="device_philox", env_mode="host")),
            (half(coevo_rng="device_philox", coevo_env="host"), {}),
            (half(), dict(rng="device_philox", dist_ctx=rank1)),                # a shard other than (0, 1)
            (half(coevo_rng="device_philox"), dict(dist_ctx=rank0)),            # rank 0 of 2: it carries a gather
        ]
        if calls is _es_calls:
            cases += [(half(coevo_antithetic=True), dict(rng="device_philox")),
                      (half(coevo_rng="device_philox", coevo_centered_rank=True), {})]
        for args, kw in cases:
            for call in calls(args, **kw):
                with pytest.raises(ValueError, match=msg):
                    call()
        for call in calls(Bag(precision="bfloat16"), rng="device_philox"):
            with pytest.raises(ValueError, match="Unsupported precision: bfloat16"):
                call()
    # what the existing suite pins, unchanged
    from tests.test_fp16_cpu import test_out_of_scope_float16_combinations_raise
    monkeypatch.undo()
    test_out_of_scope_float16_combinations_raise()


def test_the_per_call_es_helpers_stay_float32_only():
    from coevonet_amd import evolutionary_strategy as es
    with pytest.raises(ValueError, match="Unsupported precision"):
        es.get_numpy_dtype("float16")


# ------------------------------------------------------------------------------------------------------ launch scripts
def record(run):
    """run() under the golden recorder (tests/golden/make_golden_launches.py) -> its records; the job array of a float16
    multi launch is recorded field by field, as the recorder does for the float32 ones"""
    with mg.stubbed():
        plain = L.call

        def call(name, *args):
            if name in JOB_ARRAYS:
                jobs = (getattr(L, JOB_ARRAYS[name]) * int(args[1])).from_address(args[0].value)
                args = (jobs,) + args[1:]
            plain(name, *args)
        L.call = call
        mg.REC.log, mg.REC.engine, mg.REC.es, mg.REC.n_ro = [], None, False, 0
        run()
        log = mg.REC.log
    mg.REC.log = []
    return log


def calls_of(log, *names):
    return [r for r in log if r[0] == "call" and r[1] in names]


def ga_script(pop, hof, elites, **kw):
    from coevonet_amd.ga_half import HalfGAEngine

    def run():
        eng = mg.REC.engine = HalfGAEngine(pop, hof, elites, 40, 30, device="cpu", **kw)
        for gen in range(2):
            eng.rollout(gen)
            eng.select()
            eng.breed(gen, mg.SIG3)
        eng.eval_only(1)
    return record(run)


def es_script(pop, sharing, upload=False, **kw):
    import numpy as np

    from coevonet_amd.es_half import HalfESEngine

    def run():
        eng = mg.REC.engine = HalfESEngine(pop, 40, 30, device="cpu", **kw)
        for gen in range(2):
            eng.perturb(gen, mg.SIG3, sharing)
            eng.rollout(gen)
            if upload:
                eng.upload("agent_1", "pert", 0, np.zeros((pop, 1), dtype=np.float32))
            eng.update(gen, mg.LR, sharing)
            eng.evaluate(gen)
    return record(run)


def job_of_perturb_call(c):
    """the record of one coevo_fc16_perturb_dist call -> (the job's fields, (seed, flags, gen_dev))"""
    (parent, idx, child, first, n, D, sigma, seed, slo, shi, flags, gen_dev, ref, part) = c[2:]
    return (dict(parent_slab=parent, parent_idx=idx, child_slab=child, sigma_dev=sigma, dist_ref=ref, dist_partial=part,
                 child_first=first, n_children=n, D=D, stream_lo_first=slo, stream_hi=shi, pad=0), (seed, flags, gen_dev))


def job_of_finalize_call(c):
    part, n_blocks, n, dist, first, head = c[2:]
    return dict(dist_partial=part, dist=dist, head=head, n_blocks=n_blocks, n=n, first=first, pad=0)


def test_default_engines_name_no_multi_entry():
    for log in (ga_script(5, 3, 2), es_script(3, False), es_script(3, True), es_script(3, True, upload=True)):
        assert log and not [r for r in log if r[0] == "call" and "_multi" in r[1]]
    assert len(calls_of(ga_script(5, 3, 2), "coevo_fc16_perturb_dist")) == 6   # three roles, two generations


def test_multi_ga_engine_breeds_with_one_launch_each_over_the_per_role_jobs():
    plain, multi = ga_script(5, 3, 2), ga_script(5, 3, 2, multi_breed=True)
    singles = ("coevo_fc16_perturb_dist", "coevo_fc16_distance_finalize")
    # everything but the children / their distances is enqueued as before, in the same order
    strip = lambda log: [r for r in log if not (r[0] == "call" and r[1] in singles + NEW)]   # noqa: E731
    gen0 = [r for r in calls_of(plain, "coevo_fc16_distance_finalize") if r[6] == 0]   # select() of generation 0: first 0
    assert len(gen0) == 3
    assert strip(multi) == strip(plain)
    assert not calls_of(multi, "coevo_fc16_perturb_dist")
    assert calls_of(multi, "coevo_fc16_distance_finalize") == gen0
    mp, mf = calls_of(multi, NEW[0]), calls_of(multi, NEW[1])
    assert len(mp) == 2 and len(mf) == 2, "one multi perturb and one multi finalize per breed()"
    pp = calls_of(plain, "coevo_fc16_perturb_dist")
    pf = [r for r in calls_of(plain, "coevo_fc16_distance_finalize") if r not in gen0]
    for gen in range(2):
        jobs, rest = zip(*[job_of_perturb_call(c) for c in pp[3 * gen:3 * gen + 3]])
        assert len(set(rest)) == 1 and rest[0][1:] == (0, None)
        assert mp[gen][2:] == [list(jobs), 3, rest[0][0], 0, None]
        assert mf[gen][2:] == [[job_of_finalize_call(c) for c in pf[3 * gen:3 * gen + 3]], 3]
        assert all(j["head"] is not None and j["first"] == 1 for j in mf[gen][2])
    # the order inside a breed(): the promotion, the children, their distances
    names = [r[1] for r in multi if r[0] == "call"]
    i = names.index(NEW[0])
    assert names[i - 1] == "coevo_ga16_promote" and names[i + 1] == NEW[1]


@pytest.mark.parametrize("sharing", [False, True])
def test_multi_es_engine_perturbs_with_one_launch_over_the_per_role_jobs(sharing):
    plain, multi = es_script(3, sharing), es_script(3, sharing, multi_breed=True)
    singles = ("coevo_fc16_perturb_dist", "coevo_fc16_distance_finalize")
    strip = lambda log: [r for r in log if not (r[0] == "call" and r[1] in singles + NEW)]   # noqa: E731
    assert strip(multi) == strip(plain)
    assert not calls_of(multi, *singles)
    mp, mf = calls_of(multi, NEW[0]), calls_of(multi, NEW[1])
    pp, pf = calls_of(plain, singles[0]), calls_of(plain, singles[1])
    assert len(mp) == 2 and len(pp) == 6 and len(mf) == (2 if sharing else 0) and len(pf) == (6 if sharing else 0)
    for gen in range(2):
        jobs, rest = zip(*[job_of_perturb_call(c) for c in pp[3 * gen:3 * gen + 3]])
        assert len(set(rest)) == 1 and rest[0][1:] == (1, None), "COEVO_PERTURB_SKIP_LAYERNORM, no device generation"
        assert mp[gen][2:] == [list(jobs), 3, rest[0][0], 1, None]
        assert all(j["child_first"] == 0 and j["parent_idx"] == "zero_idx+0" for j in jobs)
        assert all((j["dist_ref"] is not None) == sharing and (j["dist_ref"] == j["parent_slab"]) == sharing for j in jobs)
        if sharing:
            assert mf[gen][2:] == [[job_of_finalize_call(c) for c in pf[3 * gen:3 * gen + 3]], 3]


def test_multi_es_engine_falls_back_to_per_role_distances_when_the_fused_partials_are_stale():
    """nets uploaded between perturb() and update(): the partials no longer describe the slab, so update() takes the
    standalone distance and the per-role finalize, as the default engine does"""
    plain, multi = es_script(3, True, upload=True), es_script(3, True, upload=True, multi_breed=True)
    assert not calls_of(multi, NEW[1])
    for name in ("coevo_fc16_distance", "coevo_fc16_distance_finalize"):
        assert calls_of(multi, name) == calls_of(plain, name) and len(calls_of(multi, name)) == 6
