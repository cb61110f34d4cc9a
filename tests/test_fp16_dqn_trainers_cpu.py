"""The float16 DeepQN trainers and the fused float16 env step without a GPU: every refusal of DQNGATrainer / DQNESTrainer /
dqn_*_train / the public *_train dispatchers before anything is read, drawn or loaded, and the route under the golden recorder -
float16 builds the half engines and names no float32 DeepQN entry point, float32 records the script it recorded before the
trainers read ``args.precision`` (tests/golden/dqn_trainer_launch_scripts.json).  (The two new symbols in the header, the
library and the binding: tests/test_abi.py.)"""
import re
import types

import pytest
import torch

from coevonet_amd import lib as L
from tests.golden import make_golden_dqn_trainer_scripts as mt
from tests.golden import make_golden_launches as mg
from tests.util import load_golden



class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------------------ refusals
GA_MSG, ES_MSG = "^DeepQN Co-GA training with precision float16", "^DeepQN Co-ES with precision float16"


def _ga_calls(args, **kw):
    from coevonet_amd import dqn_population as dp
    from coevonet_amd import genetic_algorithm as ga
    return (lambda: dp.DQNGATrainer(None, args, **kw), lambda: dp.dqn_genetic_algorithm_train(None, None, args, None, **kw),
            lambda: ga.genetic_algorithm_train(None, None, args, None, **kw))


def _es_calls(args, **kw):
    from coevonet_amd import dqn_population as dp
    from coevonet_amd import evolutionary_strategy as es
    return (lambda: dp.DQNESTrainer(None, args, **kw), lambda: dp.dqn_evolution_strategy_train(None, args, None, **kw),
            lambda: es.evolution_strategy_train(None, args, None, **kw))


def test_every_refusal_comes_first(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    monkeypatch.delenv("COEVO_DQN_FRAMES", raising=False)
    gathers = dict(gather_ga2=lambda eng: None, gather_es=lambda eng, what: None)
    rank1, rank0 = types.SimpleNamespace(rank=1, world=2, **gathers), types.SimpleNamespace(rank=0, world=2, **gathers)
    half = lambda **kw: Bag(precision="float16", game="pong_v3", **kw)   # noqa: E731 - nothing else may be read first
    torch.manual_seed(77)
    rng = torch.random.get_rng_state()
    n = 0
    for calls, msg in ((_ga_calls, GA_MSG), (_es_calls, ES_MSG)):
        cases = [(half(), dict(dist_ctx=rank1), {}),                      # a shard other than (0, 1)
                 (half(), dict(dist_ctx=rank0), {}),                      # rank 0 of 2: it carries a gather
                 (half(coevo_frames="host"), {}, {}),
                 (half(), {}, {"COEVO_DQN_FRAMES": "host"})]
        if calls is _es_calls:
            cases += [(half(coevo_antithetic=True), {}, {}), (half(coevo_centered_rank=True), {}, {})]
        for args, kw, env in cases:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            for call in calls(args, **kw):
                with pytest.raises(ValueError, match=msg):
                    call()
                n += 1
            for k in env:
                monkeypatch.delenv(k)
        for call in calls(Bag(precision="bfloat16", game="pong_v3")):
            with pytest.raises(ValueError, match="^Unsupported precision: bfloat16$"):
                call()
            n += 1
    assert n == 3 * (4 + 6) + 6
    assert torch.equal(torch.random.get_rng_state(), rng), "a refusal advanced the torch generator"


# --------------------------------------------------------------------------------------------------------------- route
FP32_DQN = re.compile(r"coevo_dqn_(?!es16_)")   # every float32 DeepQN entry point (coevo_dqn_es16_* are float16 ones)


def call_names(log):
    return [r[1] for r in log if r[0] == "call"]


def test_float32_trainers_record_the_script_they_recorded_before_they_read_the_precision():
    want = load_golden("dqn_trainer_launch_scripts.json")["cases"]
    assert sorted(want) == sorted(mt.CASES)
    got = mt.mint()
    assert mg.first_difference(got, want) is None
    for case, log in got.items():
        assert any(FP32_DQN.match(nm) for nm in call_names(log)), case
    # ... and a missing precision attribute is float32
    from coevonet_amd import population
    assert population.dqn_half_route(Bag(game="pong_v3"), "x", None, None, "gather_ga2") is False


@pytest.mark.parametrize("collect", [True, False])
def test_float16_co_ga_trainer_builds_the_half_engine(collect):
    log, engine = mt.record("ga", "float16", collect=collect)
    assert engine == "HalfDQNGAEngine"
    names = call_names(log)
    assert names and not [nm for nm in names if FP32_DQN.match(nm)], "a float32 DeepQN entry point in the float16 route"
    assert names.count("coevo_dqn16_perturb_dist") == 4 and names.count("coevo_dqn16_distance") == 2
    assert [r[1] for r in log if r[0] == "ro.new"] == ["HalfSynthRollout"]
    assert [r for r in log if r[0] == "ro.new"][0][-1] is False, "the fp16 slab has no tiled fc1"
    # the trainer's own steps over the half engine are the float32 trainer's: the same rollout calls and uploads, in order
    log32, engine32 = mt.record("ga", "float32", collect=collect)
    assert engine32 == "DQNGAEngine"
    other = lambda lg: [r for r in lg if r[0] in ("ro", "upload", "graph.capture", "graph.replay")]   # noqa: E731
    assert other(log) == other(log32)


@pytest.mark.parametrize("sharing", [False, True])
def test_float16_co_es_trainer_builds_the_half_engine(sharing):
    log, engine = mt.record("es", "float16", fitness_sharing=sharing)
    assert engine == "HalfDQNESEngine"
    names = call_names(log)
    assert names and not [nm for nm in names if FP32_DQN.match(nm)], "a float32 DeepQN entry point in the float16 route"
    for name, count in (("coevo_dqn16_perturb_dist", 4), ("coevo_es16_fitness", 4), ("coevo_dqn_es16_partial", 4),
                        ("coevo_dqn_es16_apply", 4), ("coevo_sharing_score", 4 if sharing else 0)):
        assert names.count(name) == count, name
    assert [r[3] for r in log if r[0] == "ro.new"] == ["HalfSynthRollout", "HalfSynthRollout"]
    assert [r for r in log if r[0] == "upload"] == [["upload", "first_0", "base", 0, 1], ["upload", "second_0", "base", 0, 1]]


def test_half_values_rounds_as_torch_rounds_a_module_to_half():
    from coevonet_amd.dqn_population import half_values
    x = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.9, 65520.0, -1e-8, 6e-8, float("inf")]).numpy()
    got = half_values(x)
    assert got.dtype == x.dtype and got.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -9, 65504.0, float("inf"), -0.0, 2.0 ** -24,
                                                     float("inf")]


# ------------------------------------------------------------------------------------------- the rollout's launch sequence
class _NamesOnly:
    """stands in for the loaded library: every entry point records its name and arguments and returns 0"""

    def __init__(self, real):
        self.real, self.log = real, []

    def __getattr__(self, name):
        if name in ("coevo_dqn16_workspace_bytes", "coevo_dqn_workspace_bytes"):
            return getattr(self.real, name)

        def entry(*args):
            assert len(args) == len(L._SIGS[name][1]), name
            self.log.append((name, args))
            return 0
        return entry


@pytest.mark.parametrize("knob,fused", [(None, True), ("1", True), ("0", False)])
def test_half_rollout_enqueues_three_launches_per_agent_step(monkeypatch, knob, fused):
    """default and COEVO_DQN16_FUSED_OUT=1: coevo_synth_step at t = 0 only, then per agent-step coevo_dqn16_out_synth_step (one
    launch) + coevo_dqn16_forward_hidden (two); =0: the four-launch route.  The fused env step reads the tasks and rows of the
    parity that acted and writes the frames of the one that acts next"""
    from coevonet_amd.dqn_ga_half import HalfSynthRollout
    if knob is None:
        monkeypatch.delenv("COEVO_DQN16_FUSED_OUT", raising=False)
    else:
        monkeypatch.setenv("COEVO_DQN16_FUSED_OUT", knob)
    fake = _NamesOnly(L.load())
    monkeypatch.setattr(L, "load", lambda: fake)
    monkeypatch.setattr(L, "_p", lambda t: None if t is None else t.data_ptr())
    slab = torch.zeros(64, dtype=torch.int32)
    ro = HalfSynthRollout([(0, 2), (1, 2), (0, 2)], [0, 16, 32], [5, 6, 7], 4, 6, slab, 123, 0, "cpu")
    assert ro.fused_out is fused
    T, ln = 3, ro.lanes[0]
    ro._enqueue_lane(ln, T, None, 0, False)
    names = [nm for nm, _ in fake.log]
    if not fused:
        assert names == ["coevo_synth_step", "coevo_dqn16_forward_argmax"] * T + ["coevo_synth_step"]
        return
    assert names == ["coevo_synth_step"] + ["coevo_dqn16_forward_hidden", "coevo_dqn16_out_synth_step"] * T
    for t in range(1, T + 1):
        a = fake.log[2 * t][1]
        q, p = (t - 1) & 1, t & 1
        assert a[6] == t and a[8] == ln["rows"][q].data_ptr() and a[9] == ln["actions"][q].data_ptr()
        assert a[10] == (ln["rows"][p].data_ptr() if t < T else None) and a[11] == (ln["frames"].data_ptr() if t < T else None)
        assert a[15] == slab.data_ptr() and a[16] == ln["tasks"][q].data_ptr() and a[17] == ln["n_tasks"][q] and a[18] == 3
        assert a[19] == ln["ws"].data_ptr() and a[20] == ro.status.data_ptr()
        h = fake.log[2 * t - 1][1]
        assert h[1] == ln["tasks"][(t - 1) & 1].data_ptr() and h[8] == ro.status.data_ptr() and h[9] == ln["ws"].data_ptr()
