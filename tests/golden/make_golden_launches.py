#!/usr/bin/env python3
"""Mint ga_launch_scripts.json: the ordered launch scripts of the four Co-GA engines (GAEngine, HalfGAEngine, DQNGAEngine,
HalfDQNGAEngine) - every C-ABI call with every argument, the calls on the rollout object and the gather callbacks in between.
Needs libcoevo.so (strides and block counts come from it) and no GPU: the engines are constructed on the CPU, ``lib.call`` is
replaced by a recorder, ``lib._p`` by the plain ``data_ptr()``, and the rollout classes by stubs that record what is asked of
them (``RolloutPlan`` keeps only n_games).

    python tests/golden/make_golden_launches.py       # writes tests/golden/ga_launch_scripts.json

The fixture was minted at the commit BEFORE population.CoGATail existed, when every engine wrote its generation tail out on
its own.  DO NOT REGENERATE it from a tree that has CoGATail: in such a tree this script only CHECKS (as does
tests/test_ga_launch_scripts_cpu.py): it replays the same driver and compares record by record.

A record is a list: ["call", entry point, arguments...], ["ro", method, arguments...], ["ro.new", class, ...] (the tables a
DeepQN rollout is constructed with), ["upload", role, region, first, n], ["gather"] / ["gather_packed"], ["torch", ...].
Integers and floats are stored as they are; a pointer as "<engine attribute>[key]+<byte offset>" resolved against the engine's tensors ("ro." in
front: the rollout's); ctypes structures (by value, by reference, and the arrays GaSelectRole / GaPromoteRole / PerturbJob /
FinalizeJob) field by field.

Stubbed the same way in every tree: ``SlabIO.upload`` (records, moves nothing), ``torch.cuda.current_stream`` /
``torch.cuda.synchronize`` (no-ops).  torch's ``copy_`` / ``fill_`` into an engine tensor are recorded between the calls
(["torch", method, destination, elements, source]); its indexed assignments are not.  The pipelined cohort path
(replay_generation_pipelined, step_sharded with K > 1) and graph capture need real streams: the GPU tests carry them.
"""
import contextlib
import ctypes as ct
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FIXTURE = os.path.join(HERE, "ga_launch_scripts.json")
ENV_KNOBS = ("COEVO_PACKED_EXCHANGE", "COEVO_PIPELINED", "COEVO_HEAVY_ROWS", "COEVO_HOST_COHORTS", "COEVO_DQN_COHORTS",
             "COEVO_DQN_FC1_LAYOUT", "COEVO_PERSISTENT", "COEVO_RESIDENT_MB", "COEVO_FRAME_COHORTS")


class Recorder:
    def __init__(self):
        self.log, self.engine = [], None

    # ---- pointers -> "<attribute>[key]+<offset>"
    def _tensors(self):
        def walk(prefix, obj):
            for name, v in sorted(vars(obj).items()):
                if torch.is_tensor(v):
                    yield prefix + name, v
                elif isinstance(v, dict):
                    for k, t in v.items():
                        if torch.is_tensor(t):
                            yield f"{prefix}{name}[{k}]", t
                elif isinstance(v, (list, tuple)):
                    for k, t in enumerate(v):
                        if torch.is_tensor(t):
                            yield f"{prefix}{name}[{k}]", t
        eng = self.engine
        if eng is not None:
            yield from walk("", eng)
            if getattr(eng, "ro", None) is not None:
                yield from walk("ro.", eng.ro)

    def ptr(self, p, must=True):
        if p is None or p == 0:
            return None
        best = None
        for name, t in self._tensors():
            off = p - t.data_ptr()
            if 0 <= off < t.numel() * t.element_size():
                best = min(best, (off, name)) if best else (off, name)
        if best is None:
            if must:
                raise AssertionError(f"pointer {p:#x} is inside none of the engine's tensors")
            return None
        return f"{best[1]}+{best[0]}"

    # ---- values
    def struct(self, s):
        out = {}
        for name, typ in s._fields_:
            v = getattr(s, name)
            out[name] = self.ptr(v) if typ is ct.c_void_p else self.value(v)
        return out

    def value(self, v):
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, (np.integer, np.floating)):
            return v.item()
        if torch.is_tensor(v):
            return self.ptr(v.data_ptr())
        if isinstance(v, np.ndarray):
            return v.tolist()
        if isinstance(v, ct.Structure):
            return self.struct(v)
        if isinstance(v, ct.Array):
            return [self.value(x) for x in v]
        if hasattr(v, "_obj"):   # ctypes.byref(...)
            return self.value(v._obj)
        if isinstance(v, (list, tuple)):
            return [self.value(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self.value(x) for k, x in v.items()}
        raise AssertionError(f"cannot record a {type(v).__name__}")

    def call(self, name, *args):
        from coevonet_amd import lib as L
        sig = L._SIGS[name][1]
        assert len(args) == len(sig) - 1, (name, len(args), len(sig))   # (+ the stream, which lib.call appends)
        arrays = {"coevo_fc_perturb_dist_multi": L.PerturbJob, "coevo_fc_distance_finalize_multi": L.FinalizeJob,
                  "coevo_fc_distance_finalize_multi_tick": L.FinalizeJob}
        rec = ["call", name]
        for i, (a, typ) in enumerate(zip(args, sig)):
            if isinstance(a, ct.c_void_p) and i == 0 and name in arrays:   # ctypes.cast(jobs, c_void_p): args[1] jobs
                a = (arrays[name] * int(args[1])).from_address(a.value)
            if typ is ct.c_void_p and (a is None or isinstance(a, int)):
                rec.append(self.ptr(a))
            else:
                rec.append(self.value(a))
        self.log.append(rec)

    def ro(self, method, *args, **kw):
        self.log.append(["ro", method] + [self.value(a) for a in args] + ([self.value(kw)] if kw else []))


REC = Recorder()


def _ro_method(name):
    def f(self, *a, **k):
        REC.ro(name, *a, **k)
    return f


def _device_rollout_init(self, plan, slab, env_seed=0, **kw):
    from coevonet_amd import lib as L
    n = plan.n_games
    self.rewards = torch.zeros(n, 3, dtype=torch.float64)
    self.state = torch.zeros(n, L.MPE_STATE_DOUBLES, dtype=torch.float64)
    self.status = torch.zeros(1, dtype=torch.int32)
    self.rng = L.PCG64State.from_seed(env_seed)
    self.use_graph, self.time_light, self.n_cohorts, self.ctx = False, False, 1, None
    self.desc = types.SimpleNamespace(merged=1)


def _synth_rollout_init(self, game_nets, net_off, ordinal0, C, n_actions, slab, env_seed, ordinals_per_gen, device="cuda",
                        bounds=None, fc1_tiled=False):
    self.n_games = n = len(game_nets)
    self.lanes = [{}] * (1 if bounds is None else len(bounds) - 1)
    self.acc = torch.zeros(n, 3, dtype=torch.float64)
    self.status = torch.zeros(1, dtype=torch.int32)
    REC.log.append(["ro.new", type(self).__name__, REC.value(np.asarray(game_nets)), [int(x) for x in net_off],
                    [int(x) for x in ordinal0], C, n_actions, int(env_seed), int(ordinals_per_gen), REC.value(bounds),
                    bool(fc1_tiled)])


def _torch_method(name):
    """torch's in-place copies and fills INTO an engine tensor, in order with the calls (the source: its name, or the number)"""
    orig = getattr(torch.Tensor, name)

    def f(self, src, *a, **k):
        dst = REC.ptr(self.data_ptr(), must=False) if REC.engine is not None and self.numel() else None
        if dst is not None:
            what = REC.ptr(src.data_ptr(), must=False) if torch.is_tensor(src) else REC.value(src)
            REC.log.append(["torch", name, dst, self.numel(), what])
        return orig(self, src, *a, **k)
    return f


def _plan_init(self, game_nets, net_off, net_D, **kw):
    self.n_games = len(game_nets)


def _upload(self, role, region, first, flat_np):
    REC.log.append(["upload", role, region, int(first), int(np.asarray(flat_np).shape[0])])
    self._uploaded(region)


@contextlib.contextmanager
def stubbed():
    """the library's call / _p, the rollout classes, SlabIO.upload and the stream calls replaced; everything put back on exit"""
    from coevonet_amd import dqn_ga_half, dqn_population, lib as L, population, rollout
    ro_methods = ("set_limits", "enqueue", "reset_segments", "reset", "run", "check_status", "collect_stamps", "close")
    patches = [(L, "call", REC.call), (L, "_p", lambda t: None if t is None else t.data_ptr()),
               (rollout.RolloutPlan, "__init__", _plan_init), (population.SlabIO, "upload", _upload),
               (torch.cuda, "current_stream", lambda *a, **k: types.SimpleNamespace(synchronize=lambda: None, cuda_stream=0)),
               (torch.cuda, "synchronize", lambda *a, **k: None),
               (torch.Tensor, "copy_", _torch_method("copy_")), (torch.Tensor, "fill_", _torch_method("fill_"))]
    for cls in (rollout.DeviceRollout, rollout.HostEnvRollout):
        patches += [(cls, "__init__", _device_rollout_init), (cls, "__del__", lambda self: None)]
        patches += [(cls, m, _ro_method(m)) for m in ro_methods]
    for cls in (dqn_population.SynthRollout, dqn_ga_half.HalfSynthRollout):
        patches += [(cls, "__init__", _synth_rollout_init), (cls, "__del__", lambda self: None)]
        patches += [(cls, m, _ro_method(m)) for m in ("set_limits", "enqueue", "close")]
    missing = object()
    saved = [(o, n, o.__dict__.get(n, missing)) for o, n, _ in patches]
    env = {k: os.environ.pop(k) for k in ENV_KNOBS if k in os.environ}
    try:
        for o, n, v in patches:
            setattr(o, n, v)
        yield
    finally:
        for o, n, v in reversed(saved):
            if v is missing:
                delattr(o, n)
            else:
                setattr(o, n, v)
        os.environ.update(env)
        REC.engine = None


# ------------------------------------------------------------------------------------------------------- the cases
SIG3 = {"agent_0": 0.05, "agent_1": 0.04, "adversary_0": 0.03}
LOOP_ARGS = types.SimpleNamespace(mutation_power_agent_0=0.05, mutation_power_agent_1=0.04, mutation_power_adversary=0.03,
                                  min_mutation_power=0.001, max_mutation_power=0.2, adaptive=True)


def _gather(eng):
    REC.log.append(["gather"])


def _gather_packed(eng):
    REC.log.append(["gather_packed"])


def _ga(pop, hof, elites, shard=(0, 1), packed=False):
    from coevonet_amd.genetic_algorithm import GAEngine
    REC.engine = GAEngine(pop, hof, elites, 40, 30, device="cpu", rng="device_philox", env="device", shard=shard,
                          gather=_gather if shard[1] > 1 else None, gather_packed=_gather_packed if packed else None)
    return REC.engine


def ga_host(pop, hof, elites, shard=(0, 1), schedule=False):
    """the host-driven generation: [rollout] select breed_device, twice (the second round finds _dist_current set on the
    fused path; a sharded generation 1 rebuilds the elites), [then the flush of the last evaluation games]"""
    eng = _ga(pop, hof, elites, shard)
    for gen in range(2):
        if schedule:
            eng.rollout(gen, with_prev_eval=gen > 0)
        eng.select()
        eng.breed_device(gen, SIG3)
    if schedule:
        eng.eval_only(1)


def ga_device_loop(pop, hof, elites):
    eng = _ga(pop, hof, elites)
    eng.setup_device_loop(LOOP_ARGS, 16)
    for gen in range(2):
        eng.replay_generation(gen)   # (the stub rollout has use_graph False: the limits, then enqueue_generation)


def ga_sharded_loop(pop, hof, elites, shard, packed=False):
    eng = _ga(pop, hof, elites, shard, packed)
    eng.setup_device_loop(LOOP_ARGS, 16)
    for gen in range(2):
        eng.step_sharded(gen)


def ga_half(pop, hof, elites):
    from coevonet_amd.ga_half import HalfGAEngine
    eng = REC.engine = HalfGAEngine(pop, hof, elites, 40, 30, device="cpu")
    for gen in range(2):
        eng.rollout(gen)
        eng.select()
        eng.breed(gen, SIG3)
    eng.eval_only(1)


def dqn(half, pop, shard=(0, 1)):
    from coevonet_amd.dqn_ga_half import HalfDQNGAEngine
    from coevonet_amd.dqn_population import ROLES2, DQNGAEngine
    kw = dict(shard=shard, gather=_gather) if shard[1] > 1 else {}
    eng = REC.engine = (HalfDQNGAEngine if half else DQNGAEngine)(pop, 2, min(2, pop), 4, 6, 5, 4, device="cpu", **kw)
    eng.load_initial({r: np.zeros((pop, 1), dtype=np.float32) for r in ROLES2},
                     {r: np.zeros((2, 1), dtype=np.float32) for r in ROLES2})
    eng.step(use_graph=False)
    eng.step(use_graph=False)
    eng.eval_only()


CASES = {
    "ga_host_fused": lambda: ga_host(5, 3, 2, schedule=True),
    "ga_host_unfused_elites": lambda: ga_host(10, 2, 9),
    "ga_host_unfused_hof": lambda: ga_host(5, 17, 2),
    "ga_host_shard_1_of_2": lambda: ga_host(6, 2, 2, shard=(1, 2)),
    "ga_host_shard_0_of_2": lambda: ga_host(6, 2, 2, shard=(0, 2)),
    "ga_device_loop_fused": lambda: ga_device_loop(5, 3, 2),
    "ga_device_loop_unfused": lambda: ga_device_loop(10, 2, 9),
    "ga_sharded_loop_0_of_2": lambda: ga_sharded_loop(6, 2, 2, (0, 2)),
    "ga_sharded_loop_1_of_2": lambda: ga_sharded_loop(6, 2, 2, (1, 2)),
    "ga_sharded_loop_packed_0_of_2": lambda: ga_sharded_loop(6, 2, 2, (0, 2), packed=True),
    "ga_sharded_loop_packed_1_of_2": lambda: ga_sharded_loop(6, 2, 2, (1, 2), packed=True),
    "ga_sharded_loop_unfused_1_of_2": lambda: ga_sharded_loop(20, 2, 9, (1, 2)),
    "ga_sharded_loop_only_the_best": lambda: ga_sharded_loop(2, 1, 1, (0, 2)),
    "ga_half": lambda: ga_half(5, 3, 2),
    "dqn_ga": lambda: dqn(False, 3),
    "dqn_ga_shard_1_of_2": lambda: dqn(False, 4, (1, 2)),
    "dqn_ga_shard_0_of_2": lambda: dqn(False, 4, (0, 2)),
    "dqn_ga_pop_1": lambda: dqn(False, 1),
    "dqn_ga_half": lambda: dqn(True, 3),
    "dqn_ga_half_pop_1": lambda: dqn(True, 1),
}


def mint():
    out = {}
    with stubbed():
        for name, run in CASES.items():
            REC.log, REC.engine = [], None
            run()
            out[name] = REC.log
    REC.log = []
    return json.loads(json.dumps(out))


def first_difference(got, want):
    """-> None, or (case, record index, got record, wanted record) of the first record that differs"""
    for case in sorted(set(got) | set(want)):
        g, w = got.get(case, []), want.get(case, [])
        for i in range(max(len(g), len(w))):
            a, b = (g[i] if i < len(g) else None), (w[i] if i < len(w) else None)
            if a != b:
                return case, i, a, b
    return None


if __name__ == "__main__":
    from coevonet_amd import population
    got = mint()
    if hasattr(population, "CoGATail"):
        with open(FIXTURE) as f:
            want = json.load(f)["cases"]
        bad = first_difference(got, want)
        print("check only (population.CoGATail exists):", "the engines replay the fixture's launch scripts" if bad is None
              else "DIFFERENT from the fixture: case %s record %d\n  got  %s\n  want %s" % bad)
        sys.exit(0 if bad is None else 1)
    with open(FIXTURE, "w") as f:
        json.dump({"header": "launch scripts of the Co-GA engines before population.CoGATail (make_golden_launches.py); "
                             "the pipelined cohort path and graph capture are left to the GPU tests",
                   "cases": got}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes;", {k: len(v) for k, v in got.items()})
