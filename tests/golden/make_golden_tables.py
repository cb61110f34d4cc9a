#!/usr/bin/env python3
"""Mint engine_tables.json: what the four fully connected engines hand to ``RolloutPlan`` (games, net_off, net_D, and the
evaluation games of Co-ES) with their slab layout (base, strides, slab length) and n_main.  Needs libcoevo.so (the strides
come from it) and no GPU: the engines are constructed on the CPU with ``RolloutPlan.__init__`` recording its arguments and the
rollout objects left empty.

    python tests/golden/make_golden_tables.py         # writes tests/golden/engine_tables.json

The fixture was minted at the commit BEFORE coevonet_amd/population.py existed, when every engine still built its own table:
tests/test_population_cpu.py holds the shared builders to it.  DO NOT REGENERATE it from a tree that has population.py: the
engines there take their tables from the very functions the fixture pins, so a fresh fixture could never show a drift.  In
such a tree this script only CHECKS: it constructs the engines and compares what they hand to RolloutPlan with the fixture.
The shapes are the smallest that take every branch: a Hall of Fame deeper than one (newest-first opponents, quirk Q4), a
shard with lo > 0.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from coevonet_amd import rollout  # noqa: E402

CALLS = []


def _record(self, game_nets, net_off, net_D, **kw):
    CALLS.append((np.asarray(game_nets).tolist(), [int(x) for x in net_off], [int(x) for x in net_D]))
    self.n_games = len(game_nets)


rollout.RolloutPlan.__init__ = _record
rollout.DeviceRollout.__init__ = lambda self, *a, **k: None
rollout.HostEnvRollout.__init__ = lambda self, *a, **k: None
rollout.DeviceRollout.__del__ = lambda self: None

from coevonet_amd.es_half import HalfESEngine  # noqa: E402
from coevonet_amd.evolutionary_strategy import ESEngine  # noqa: E402
from coevonet_amd.ga_half import HalfGAEngine  # noqa: E402
from coevonet_amd.genetic_algorithm import GAEngine  # noqa: E402

CASES = {
    "ga_f32": (GAEngine, dict(pop=5, hof=3, elites=2)),
    "ga_f16": (HalfGAEngine, dict(pop=5, hof=3, elites=2)),
    "ga_f32_shard": (GAEngine, dict(pop=6, hof=2, elites=2, shard=(1, 2))),
    "es_f32": (ESEngine, dict(pop=3)),
    "es_f16": (HalfESEngine, dict(pop=3)),
    "es_f32_shard": (ESEngine, dict(pop=4, shard=(1, 2))),
}


def mint():
    out = {}
    for name, (cls, kw) in CASES.items():
        del CALLS[:]
        eng = cls(device="cpu", **kw)
        rec = {"engine": cls.__name__, "args": {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()},
               "lo": int(getattr(eng, "lo", 0)), "hi": int(getattr(eng, "hi", eng.pop)),
               "stride": {r: int(s) for r, s in eng.stride.items()}, "base": eng.base, "total": int(eng.slab.numel()),
               "n_main": int(eng.n_main), "games": CALLS[0][0], "net_off": CALLS[0][1], "net_D": CALLS[0][2]}
        if len(CALLS) > 1:   # Co-ES: the evaluation plan shares the net table
            assert CALLS[1][1:] == CALLS[0][1:]
            rec["eval_games"] = CALLS[1][0]
        out[name] = rec
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "engine_tables.json")
    got = json.loads(json.dumps(mint()))
    if os.path.exists(os.path.join(REPO, "coevonet_amd", "population.py")):
        with open(path) as f:
            want = json.load(f)
        bad = [k for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)]
        print("check only (population.py exists):", "the engines hand RolloutPlan the fixture's tables" if not bad
              else f"DIFFERENT from the fixture: {bad}")
        sys.exit(1 if bad else 0)
    with open(path, "w") as f:
        json.dump(got, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")
