#!/usr/bin/env python3
"""Mint dqn_trainer_launch_scripts.json: the ordered launch scripts of ``DQNGATrainer`` and ``DQNESTrainer`` in float32 - every
C-ABI call with every argument, the calls on the rollout objects, the uploads - recorded with make_golden_launches.py's recorder
(``stubbed()``: no GPU, the engines are built on the CPU).  Needs libcoevo.so.

    python tests/golden/make_golden_dqn_trainer_scripts.py       # writes (or checks) the fixture

The fixture was minted at the commit BEFORE the trainers read ``args.precision``, when they could only build the float32
engines.  DO NOT REGENERATE it from a tree whose trainers take a precision (``population.dqn_half_route`` exists): there this
script only CHECKS it, as tests/test_fp16_dqn_trainers_cpu.py does - the float32 route must go on enqueuing the same calls with
the same arguments.

``record(kind, precision)`` also serves the float16 trainers of such a tree (no fixture: their engines have their own)."""
import contextlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

from tests.golden import make_golden_launches as mg  # noqa: E402
from tests.util import Bag  # noqa: E402

FIXTURE = os.path.join(HERE, "dqn_trainer_launch_scripts.json")
ENGINES = {"ga": (("dqn_population", "DQNGAEngine"), ("dqn_ga_half", "HalfDQNGAEngine")),
           "es": (("dqn_population", "DQNESEngine"), ("dqn_es_half", "HalfDQNESEngine"))}
CASES = {"dqn_ga_trainer": ("ga", {}), "dqn_ga_trainer_no_collect": ("ga", {"collect": False}),
         "dqn_es_trainer": ("es", {}), "dqn_es_trainer_sharing": ("es", {"fitness_sharing": True})}


@contextlib.contextmanager
def _engines_on_the_cpu():
    """the trainers build their engine on "cuda": build it on the CPU and hand it to the recorder, which names pointers by the
    engine's tensors"""
    import importlib
    saved = []
    for pair in ENGINES.values():
        for mod_name, cls_name in pair:
            mod = importlib.import_module("coevonet_amd." + mod_name)
            real = getattr(mod, cls_name)

            def make(*a, _real=real, **k):
                eng = mg.REC.engine = _real(*a, device="cpu", **k)
                return eng
            saved.append((mod, cls_name, real))
            setattr(mod, cls_name, make)
    try:
        yield
    finally:
        for mod, cls_name, real in saved:
            setattr(mod, cls_name, real)


def record(kind, precision="float32", collect=True, fitness_sharing=False):
    """two generations of the trainer + finish() + close() -> (records, the engine's class name)"""
    from coevonet_amd import dqn_population as dp
    from coevonet_amd.atari_synthetic import SyntheticAtariAEC
    args = Bag(game="pong_v3", precision=precision, population=3, hof_size=2, elites_number=2, max_timesteps_per_episode=5,
               max_evaluation_steps=4, generations=2, adaptive=True, mutation_power_agent_0=0.05, mutation_power_agent_1=0.04,
               learning_rate=0.01, fitness_sharing=fitness_sharing)
    env = SyntheticAtariAEC("pong_v3", channels=4)
    env.reset(seed=123)
    torch.manual_seed(5)
    with mg.stubbed(), _engines_on_the_cpu():
        mg.REC.log, mg.REC.engine, mg.REC.es, mg.REC.n_ro = [], None, kind == "es", 0
        tr = (dp.DQNGATrainer if kind == "ga" else dp.DQNESTrainer)(env, args, collect=collect)
        for _ in range(args.generations):
            tr.step()
        tr.finish()
        tr.close()
        log, name = mg.REC.log, type(tr.eng).__name__
    mg.REC.log = []
    return json.loads(json.dumps(log)), name


def mint():
    return {case: record(kind, **kw)[0] for case, (kind, kw) in CASES.items()}


if __name__ == "__main__":
    from coevonet_amd import population
    got = mint()
    if hasattr(population, "dqn_half_route"):
        with open(FIXTURE) as f:
            want = json.load(f)["cases"]
        bad = mg.first_difference(got, want)
        print("dqn_trainer_launch_scripts.json: check only (population.dqn_half_route exists):",
              "the float32 trainers replay the fixture's launch scripts" if bad is None
              else "DIFFERENT from the fixture: case %s record %d\n  got  %s\n  want %s" % bad)
        sys.exit(0 if bad is None else 1)
    with open(FIXTURE, "w") as f:
        json.dump({"header": "launch scripts of DQNGATrainer / DQNESTrainer before they read args.precision "
                             "(make_golden_dqn_trainer_scripts.py)", "cases": got}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes;", {k: len(v) for k, v in got.items()})
