#!/usr/bin/env python3
"""Mint ga_launch_scripts.json and es_launch_scripts.json: the ordered launch scripts of the four Co-GA engines (GAEngine,
HalfGAEngine, DQNGAEngine, HalfDQNGAEngine) and of the three Co-ES engines (ESEngine, HalfESEngine, DQNESEngine) - every
C-ABI call with every argument, the calls on the rollout object and the gather callbacks in between.
Needs libcoevo.so (strides and block counts come from it) and no GPU: the engines are constructed on the CPU, ``lib.call`` is
replaced by a recorder, ``lib._p`` by the plain ``data_ptr()``, and the rollout classes by stubs that record what is asked of
them (``RolloutPlan`` keeps only n_games).

    python tests/golden/make_golden_launches.py       # writes (or checks) the two fixtures

The Co-GA fixture was minted at the commit BEFORE population.CoGATail existed, when every engine wrote its generation tail out
on its own; the Co-ES fixture at the commit BEFORE population.CoESUpdate existed, when ESEngine.update_device and
DQNESEngine.generation each wrote the update sequence out and DQNESEngine built its own game table.  DO NOT REGENERATE a
fixture from a tree that has its mixin: in such a tree this script only CHECKS it (as do tests/test_ga_launch_scripts_cpu.py
and tests/test_es_launch_scripts_cpu.py): it replays the same driver and compares record by record.

ga_cohort_launch_scripts.json (COHORT_CASES) was minted the same way at the commit BEFORE population.co_ga_reset_segments
existed: GAEngine's _breed_cohort / _reset_cohort called directly (they need no stream), its host-driven selection under
hof_mean / population_sharing and HalfGAEngine's multi-role breeding; in a tree that has the function it is only checked
(tests/test_ga_cohort_launch_scripts_cpu.py).

A record is a list: ["call", entry point, arguments...], ["ro", method, arguments...], ["ro.new", class, ...] (the tables a
DeepQN rollout is constructed with), ["upload", role, region, first, n], ["gather"] / ["gather_packed"], ["torch", ...].
Integers and floats are stored as they are; a pointer as "<engine attribute>[key]+<byte offset>" resolved against the
engine's tensors ("ro." in front: the rollout's); ctypes structures (by value, by reference, and the arrays GaSelectRole /
GaPromoteRole / PerturbJob / FinalizeJob) field by field.

Stubbed the same way in every tree: ``SlabIO.upload`` (records, moves nothing), ``torch.cuda.current_stream`` /
``torch.cuda.synchronize`` (no-ops).  torch's ``copy_`` / ``fill_`` into an engine tensor are recorded between the calls
(["torch", method, destination, elements, source]); its indexed assignments are not.  The pipelined cohort path
(replay_generation_pipelined, step_sharded with K > 1) and graph capture need real streams: the GPU tests carry them.

The Co-ES records hold more (for the ES cases only, so that the Co-GA records stay what they were): the rollout a call went to
("ro" / "eval_ro" in front, also in pointers), ``reset_from_ordinals``, the tables every plan and rollout is constructed with
(["plan.new", ...], ["ro.new", which, ...] with the length of the slab it reads; HostFrameRollout stubbed like
SynthRollout), torch's indexed assignments into an engine tensor (["setitem", destination, index, source - its name where it
is an engine tensor -, the source's shape]) and ``div_``, the gather callback with its kind (["gather", "stats" |
"partials"]), and the evaluation graph: ``population.captured`` is replaced by a stub that records ["graph.capture"] and runs nothing, whose ``replay()`` records
["graph.replay"] and runs fn() once.  The first argument of coevo_sharing_score, the float32 copy of the gathered distances
that the engine does not keep, is recorded as "tmp" (any other pointer outside the engine's tensors is an error); a small
host tensor copied into an engine tensor by its values.
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
ES_FIXTURE = os.path.join(HERE, "es_launch_scripts.json")
COHORT_FIXTURE = os.path.join(HERE, "ga_cohort_launch_scripts.json")
ENV_KNOBS = ("COEVO_PACKED_EXCHANGE", "COEVO_PIPELINED", "COEVO_HEAVY_ROWS", "COEVO_HOST_COHORTS", "COEVO_DQN_COHORTS",
             "COEVO_DQN_FC1_LAYOUT", "COEVO_PERSISTENT", "COEVO_RESIDENT_MB", "COEVO_FRAME_COHORTS", "COEVO_ES_COHORTS",
             "COEVO_DQN_EVAL_GRAPH", "COEVO_DQN_EVAL_TILED")


class Recorder:
    def __init__(self):
        self.log, self.engine = [], None
        self.es, self.n_ro = False, 0   # es: a Co-ES case (its records hold more); n_ro: rollouts constructed in this case

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
            if self.es and getattr(eng, "eval_ro", None) is not None:
                yield from walk("eval_ro.", eng.eval_ro)

    def ptr(self, p, must=True, tmp=False):
        """tmp: the one argument that may point outside every engine tensor (then recorded as "tmp")"""
        if p is None or p == 0:
            return None
        best = None
        for name, t in self._tensors():
            off = p - t.data_ptr()
            if 0 <= off < t.numel() * t.element_size():
                best = min(best, (off, name)) if best else (off, name)
        if best is None:
            if tmp:
                return "tmp"
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
        if isinstance(v, ct._SimpleCData):
            return v.value
        if isinstance(v, (list, tuple)):
            return [self.value(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self.value(x) for k, x in v.items()}
        raise AssertionError(f"cannot record a {type(v).__name__}")

    def call(self, name, *args):
        from coevonet_amd import lib as L
        sig = (L._SIGS.get(name) or L._SH_SIGS[name])[1]   # (coevo.h, or the sharing modes' header)
        assert len(args) == len(sig) - 1, (name, len(args), len(sig))   # (+ the stream, which lib.call appends)
        arrays = {"coevo_fc_perturb_dist_multi": L.PerturbJob, "coevo_fc_distance_finalize_multi": L.FinalizeJob,
                  "coevo_fc_distance_finalize_multi_tick": L.FinalizeJob,
                  "coevo_fc16_perturb_dist_multi": L.Perturb16Job, "coevo_fc16_distance_finalize_multi": L.FinalizeJob}
        rec = ["call", name]
        for i, (a, typ) in enumerate(zip(args, sig)):
            if isinstance(a, ct.c_void_p) and i == 0 and name in arrays:   # ctypes.cast(jobs, c_void_p): args[1] jobs
                a = (arrays[name] * int(args[1])).from_address(a.value)
            if typ is ct.c_void_p and (a is None or isinstance(a, int)):
                # (a Co-ES engine hands coevo_sharing_score a float32 copy of the gathered distances that it does not keep)
                rec.append(self.ptr(a, tmp=self.es and name == "coevo_sharing_score" and i == 0))
            else:
                rec.append(self.value(a))
        self.log.append(rec)

    def ro(self, method, *args, which="ro", **kw):
        self.log.append([which, method] + [self.value(a) for a in args] + ([self.value(kw)] if kw else []))

    def new_ro(self, ro):
        """a Co-ES engine constructs its training rollout first, then the evaluation rollout (checked by the ES driver)"""
        ro._rec_name = ("ro", "eval_ro")[self.n_ro] if self.es else "ro"
        self.n_ro += 1
        return ro._rec_name

    def index(self, ix):
        """the index of an indexed assignment: slices as "start:stop", tensors by name (or shape, where the engine keeps none)"""
        if isinstance(ix, tuple):
            return [self.index(x) for x in ix]
        if isinstance(ix, slice):
            assert ix.step is None
            return ":".join("" if x is None else str(int(x)) for x in (ix.start, ix.stop))
        if torch.is_tensor(ix):
            return self.ptr(ix.data_ptr(), must=False) or ["tensor"] + list(ix.shape)
        return ix if ix is None or isinstance(ix, int) else str(ix)


REC = Recorder()


def _ro_method(name):
    def f(self, *a, **k):
        REC.ro(name, *a, which=getattr(self, "_rec_name", "ro"), **k)
    return f


def _slab_id(slab):
    """the slab a rollout is constructed over (the engine is not there yet to name it): its length and words"""
    return [slab.numel(), str(slab.dtype)]


def _device_rollout_init(self, plan, slab, env_seed=0, **kw):
    from coevonet_amd import lib as L
    n = plan.n_games
    self.rewards = torch.zeros(n, 3, dtype=torch.float64)
    self.state = torch.zeros(n, L.MPE_STATE_DOUBLES, dtype=torch.float64)
    self.status = torch.zeros(1, dtype=torch.int32)
    self.rng = L.PCG64State.from_seed(env_seed)
    self.use_graph, self.time_light, self.n_cohorts, self.ctx = False, False, 1, None
    self.desc = types.SimpleNamespace(merged=1)
    which = REC.new_ro(self)
    if REC.es:
        REC.log.append(["ro.new", which, type(self).__name__, _slab_id(slab), int(env_seed), REC.value(kw)])


def _synth_rollout_init(self, game_nets, net_off, ordinal0, C, n_actions, slab, env_seed, ordinals_per_gen, device="cuda",
                        bounds=None, fc1_tiled=False):
    self.n_games = n = len(game_nets)
    self.lanes = [{}] * (1 if bounds is None else len(bounds) - 1)
    self.acc = torch.zeros(n, 3, dtype=torch.float64)
    self.status = torch.zeros(1, dtype=torch.int32)
    which = REC.new_ro(self)
    REC.log.append(["ro.new"] + ([which, _slab_id(slab)] if REC.es else [])
                   + [type(self).__name__, REC.value(np.asarray(game_nets)), [int(x) for x in net_off],
                      [int(x) for x in ordinal0], C, n_actions, int(env_seed), int(ordinals_per_gen), REC.value(bounds),
                      bool(fc1_tiled)])


def _host_frame_rollout_init(self, *a, threads=None, **k):
    _synth_rollout_init(self, *a, **k)


def _torch_method(name, es_only=False):
    """torch's in-place copies and fills INTO an engine tensor, in order with the calls (the source: its name, or the number;
    in a Co-ES case a small tensor the engine does not keep by its values)"""
    orig = getattr(torch.Tensor, name)

    def f(self, src, *a, **k):
        on = REC.engine is not None and self.numel() and (REC.es or not es_only)
        dst = REC.ptr(self.data_ptr(), must=False) if on else None
        if dst is not None:
            what = REC.ptr(src.data_ptr(), must=False) if torch.is_tensor(src) else REC.value(src)
            if what is None and REC.es and torch.is_tensor(src) and src.numel() <= 4 and name == "copy_":
                what = src.tolist()
            REC.log.append(["torch", name, dst, self.numel(), what])
        return orig(self, src, *a, **k)
    return f


def _setitem(self, ix, src):
    """an indexed assignment into an engine tensor (Co-ES cases only)"""
    dst = REC.ptr(self.data_ptr(), must=False) if REC.es and REC.engine is not None and self.numel() else None
    if dst is not None:
        tensor = torch.is_tensor(src)
        REC.log.append(["setitem", dst, REC.index(ix), REC.ptr(src.data_ptr(), must=False) if tensor else REC.value(src),
                        list(src.shape) if tensor else None])
    return _SETITEM(self, ix, src)


_SETITEM = torch.Tensor.__setitem__


class _Graph:
    def __init__(self, fn):
        self.fn = fn
        REC.log.append(["graph.capture"])

    def replay(self):
        REC.log.append(["graph.replay"])
        self.fn()


def _plan_init(self, game_nets, net_off, net_D, **kw):
    self.n_games = len(game_nets)
    if REC.es:
        REC.log.append(["plan.new", REC.value(np.asarray(game_nets)), [int(x) for x in net_off], [int(x) for x in net_D],
                        REC.value({k: v for k, v in kw.items() if k != "device" and v is not None})])   # (None: the default)


def _upload(self, role, region, first, flat_np):
    REC.log.append(["upload", role, region, int(first), int(np.asarray(flat_np).shape[0])])
    self._uploaded(region)


@contextlib.contextmanager
def stubbed():
    """the library's call / _p, the rollout classes, SlabIO.upload and the stream calls replaced; everything put back on exit"""
    from coevonet_amd import dqn_ga_half, dqn_population, lib as L, population, rollout
    ro_methods = ("set_limits", "enqueue", "reset_segments", "reset", "run", "check_status", "collect_stamps", "close",
                  "reset_from_ordinals")
    patches = [(L, "call", REC.call), (L, "_p", lambda t: None if t is None else t.data_ptr()),
               (rollout.RolloutPlan, "__init__", _plan_init), (population.SlabIO, "upload", _upload),
               (torch.cuda, "current_stream", lambda *a, **k: types.SimpleNamespace(synchronize=lambda: None, cuda_stream=0)),
               (torch.cuda, "synchronize", lambda *a, **k: None),
               (torch.Tensor, "copy_", _torch_method("copy_")), (torch.Tensor, "fill_", _torch_method("fill_")),
               (torch.Tensor, "div_", _torch_method("div_", es_only=True)), (torch.Tensor, "__setitem__", _setitem),
               (population, "captured", _Graph), (dqn_population, "captured", _Graph)]
    for cls in (rollout.DeviceRollout, rollout.HostEnvRollout):
        patches += [(cls, "__init__", _device_rollout_init), (cls, "__del__", lambda self: None)]
        patches += [(cls, m, _ro_method(m)) for m in ro_methods]
    for cls in (dqn_population.SynthRollout, dqn_ga_half.HalfSynthRollout):
        patches += [(cls, "__init__", _synth_rollout_init), (cls, "__del__", lambda self: None)]
        patches += [(cls, m, _ro_method(m)) for m in ("set_limits", "enqueue", "close")]
    patches += [(dqn_population.HostFrameRollout, "__init__", _host_frame_rollout_init),
                (dqn_population.HostFrameRollout, "__del__", lambda self: None)]
    patches += [(dqn_population.HostFrameRollout, m, _ro_method(m)) for m in ("set_limits", "enqueue", "close")]
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
        REC.engine, REC.es = None, False


# ------------------------------------------------------------------------------------------------------- the cases
SIG3 = {"agent_0": 0.05, "agent_1": 0.04, "adversary_0": 0.03}
LOOP_ARGS = types.SimpleNamespace(mutation_power_agent_0=0.05, mutation_power_agent_1=0.04, mutation_power_adversary=0.03,
                                  min_mutation_power=0.001, max_mutation_power=0.2, adaptive=True)


def _gather(eng):
    REC.log.append(["gather"])


def _gather_packed(eng):
    REC.log.append(["gather_packed"])


def _ga(pop, hof, elites, shard=(0, 1), packed=False, **kw):
    from coevonet_amd.genetic_algorithm import GAEngine
    REC.engine = GAEngine(pop, hof, elites, 40, 30, device="cpu", rng="device_philox", env="device", shard=shard,
                          gather=_gather if shard[1] > 1 else None, gather_packed=_gather_packed if packed else None, **kw)
    return REC.engine


def ga_host(pop, hof, elites, shard=(0, 1), schedule=False, **modes):
    """the host-driven generation: [rollout] select breed_device, twice (the second round finds _dist_current set on the
    fused path; a sharded generation 1 rebuilds the elites), [then the flush of the last evaluation games]"""
    eng = _ga(pop, hof, elites, shard, **modes)
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


def ga_half(pop, hof, elites, **kw):
    from coevonet_amd.ga_half import HalfGAEngine
    eng = REC.engine = HalfGAEngine(pop, hof, elites, 40, 30, device="cpu", **kw)
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


# ------------------------------------------------------------------------------------------- the cohort and sharing cases
def ga_cohorts(pop, hof, elites, cohorts, bounds, shard=(0, 1), from_counter=False):
    """what a cohort's stream is handed in the pipelined loop, generations 0..2, called directly (no stream needed): the
    deferred breeding of the cohort's children (from generation 1 on: those of generation gen - 1), then the reset of its
    games.  from_counter: the children of generation gen with the generation read from the device counter, whose tick rides
    in the distance reduction (the K = 1 tail of the packed exchange), before the reset of generation gen + 1's games."""
    eng = _ga(pop, hof, elites, shard, cohorts=cohorts)
    assert eng.K == cohorts and eng.cohort_bounds.tolist() == bounds, (eng.K, eng.cohort_bounds)
    eng.setup_device_loop(LOOP_ARGS, 16)
    for gen in range(3):
        for k in reversed(range(eng.K)):   # (the order of _enqueue_cohort_chains: the caller's stream, cohort 0, last)
            if from_counter:
                eng._reset_cohort(k, gen)
                eng._breed_cohort(k, gen, eng.gen_dev.data_ptr(), True)
            else:
                if gen > 0:
                    eng._breed_cohort(k, gen - 1)
                eng._reset_cohort(k, gen)


COHORT_CASES = {
    # cohort 0 holds individual 0 (the max(lo_k, 1) - 1 clamp, the best_dist head); the evaluation games go with the last
    # cohort from generation 1 on
    "ga_cohorts_2_of_6": lambda: ga_cohorts(6, 2, 2, 2, [0, 3, 6]),
    "ga_cohorts_2_of_6_from_counter": lambda: ga_cohorts(6, 2, 2, 2, [0, 3, 6], from_counter=True),
    "ga_cohorts_3_of_7_uneven": lambda: ga_cohorts(7, 3, 2, 3, [0, 2, 4, 7]),
    # cohort 0 holds only the unchanged best: no breeding launch, dist[0] := best_dist, the counter's tick on its own
    "ga_cohorts_only_the_best": lambda: ga_cohorts(2, 1, 1, 2, [0, 1, 2]),
    "ga_cohorts_only_the_best_from_counter": lambda: ga_cohorts(2, 1, 1, 2, [0, 1, 2], from_counter=True),
    "ga_cohorts_shard_1_of_2": lambda: ga_cohorts(12, 2, 2, 2, [0, 3, 6], shard=(1, 2)),
    # the launch-per-step selection of the two sharing modes (the second generation finds _dist_current set)
    "ga_host_hof_mean": lambda: ga_host(5, 3, 2, hof_mean=True),
    "ga_host_population_sharing": lambda: ga_host(5, 3, 2, population_sharing=True),
    "ga_host_hof_mean_population_sharing": lambda: ga_host(5, 3, 2, hof_mean=True, population_sharing=True),
    "ga_half_multi_breed": lambda: ga_half(5, 3, 2, multi_breed=True),
}


# ------------------------------------------------------------------------------------------------------- the Co-ES cases
LR = 0.01


def _gather_es(eng, what):
    REC.log.append(["gather", what])


def _es_engine(eng):
    assert eng.ro._rec_name == "ro" and eng.eval_ro._rec_name == "eval_ro" and REC.n_ro == 2
    REC.engine = eng
    return eng


def es(pop, sharing, shard=(0, 1), env="device", **kw):
    """two generations of perturb -> rollout -> update -> evaluate"""
    from coevonet_amd.evolutionary_strategy import ESEngine
    eng = _es_engine(ESEngine(pop, 40, 30, device="cpu", rng="device_philox", env=env, shard=shard,
                              gather=_gather_es if shard[1] > 1 else None, **kw))
    for gen in range(2):
        eng.perturb_device(gen, SIG3)
        eng.rollout(gen)
        eng.update_device(gen, LR, sharing)
        eng.evaluate(gen)


def es_half(pop, sharing, upload=False):
    """the same four steps; upload: nets arrive between perturb and update, so the fused distances no longer describe the slab"""
    from coevonet_amd.es_half import HalfESEngine
    eng = _es_engine(HalfESEngine(pop, 40, 30, device="cpu"))
    for gen in range(2):
        eng.perturb(gen, SIG3, sharing)
        eng.rollout(gen)
        if upload:
            eng.upload("agent_1", "pert", 0, np.zeros((pop, 1), dtype=np.float32))
        eng.update(gen, LR, sharing)
        eng.evaluate(gen)


def dqn_es(pop, sharing, shard=(0, 1), frames="device", knobs=None, **kw):
    from coevonet_amd.dqn_population import DQNESEngine
    os.environ.update(knobs or {})
    try:
        eng = _es_engine(DQNESEngine(pop, 4, 6, 5, 4, device="cpu", shard=shard, gather=_gather_es if shard[1] > 1 else None,
                                     first_ordinal=7, frames=frames, **kw))
        for gen in range(2):
            eng.generation(gen, (0.05, 0.04), LR, sharing)
    finally:
        for k in knobs or {}:
            del os.environ[k]


ES_CASES = {
    "es": lambda: es(3, False),
    "es_sharing": lambda: es(3, True),
    "es_extension": lambda: es(4, False, antithetic=True, centered_rank=True),
    "es_shard_0_of_2": lambda: es(4, True, shard=(0, 2)),
    "es_shard_1_of_2": lambda: es(4, True, shard=(1, 2)),
    "es_host_env": lambda: es(3, False, env="host"),
    "es_pop_1": lambda: es(1, True),
    "es_half": lambda: es_half(3, False),
    "es_half_sharing": lambda: es_half(3, True),
    "es_half_upload": lambda: es_half(3, True, upload=True),
    "dqn_es": lambda: dqn_es(3, False),
    "dqn_es_sharing": lambda: dqn_es(3, True),
    "dqn_es_extension": lambda: dqn_es(4, True, antithetic=True, centered_rank=True),
    "dqn_es_shard_0_of_2": lambda: dqn_es(4, True, shard=(0, 2)),
    "dqn_es_shard_1_of_2": lambda: dqn_es(4, True, shard=(1, 2)),
    "dqn_es_pop_1": lambda: dqn_es(1, True),
    "dqn_es_host_frames": lambda: dqn_es(3, True, frames="host"),
    "dqn_es_eval_on_the_slab": lambda: dqn_es(3, False, knobs={"COEVO_DQN_EVAL_TILED": "0"}),
    "dqn_es_eval_eager": lambda: dqn_es(3, True, knobs={"COEVO_DQN_EVAL_GRAPH": "0"}),
}


def mint(cases=None):
    """-> {case: records} of the Co-GA cases (default) or of the cases given"""
    cases = CASES if cases is None else cases
    out = {}
    with stubbed():
        for name, run in cases.items():
            REC.log, REC.engine, REC.es, REC.n_ro = [], None, cases is ES_CASES, 0
            run()
            out[name] = REC.log
    REC.log = []
    return json.loads(json.dumps(out))


def mint_es():
    return mint(ES_CASES)


def mint_cohorts():
    return mint(COHORT_CASES)


def first_difference(got, want):
    """-> None, or (case, record index, got record, wanted record) of the first record that differs"""
    for case in sorted(set(got) | set(want)):
        g, w = got.get(case, []), want.get(case, [])
        for i in range(max(len(g), len(w))):
            a, b = (g[i] if i < len(g) else None), (w[i] if i < len(w) else None)
            if a != b:
                return case, i, a, b
    return None


def _check_or_write(got, path, mixin, header):
    """-> exit status: in a tree that has `mixin` the fixture is only checked, else written"""
    from coevonet_amd import population
    name = os.path.basename(path)
    if hasattr(population, mixin):
        with open(path) as f:
            want = json.load(f)["cases"]
        bad = first_difference(got, want)
        print(f"{name}: check only (population.{mixin} exists):", "the engines replay the fixture's launch scripts"
              if bad is None else "DIFFERENT from the fixture: case %s record %d\n  got  %s\n  want %s" % bad)
        return 0 if bad is None else 1
    with open(path, "w") as f:
        json.dump({"header": header, "cases": got}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes;", len(got), "cases,", sum(len(v) for v in got.values()), "records;",
          {k: len(v) for k, v in got.items()})
    return 0


if __name__ == "__main__":
    status = _check_or_write(mint(), FIXTURE, "CoGATail",
                             "launch scripts of the Co-GA engines before population.CoGATail (make_golden_launches.py); "
                             "the pipelined cohort path and graph capture are left to the GPU tests")
    status |= _check_or_write(mint_es(), ES_FIXTURE, "CoESUpdate",
                              "launch scripts of the Co-ES engines before population.CoESUpdate (make_golden_launches.py); "
                              "the cohort chains of the rollouts and the real graph capture are left to the GPU tests")
    status |= _check_or_write(mint_cohorts(), COHORT_FIXTURE, "co_ga_reset_segments",
                              "launch scripts of GAEngine's cohort breeding and resets, of its selection under hof_mean / "
                              "population_sharing and of HalfGAEngine's multi-role breeding, before "
                              "population.co_ga_reset_segments (make_golden_launches.py)")
    sys.exit(status)
