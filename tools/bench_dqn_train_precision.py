#!/usr/bin/env python3
"""The float16 DeepQN rollout with the output layer fused into the env step against the four-launch route, and the float16
DeepQN trainers against the float32 ones:

    python tools/bench_dqn_train_precision.py [--repeats 9] [--warmup 3] [--settle-ms 120] [--only steps|engines|trainers]
                                              [--out FILE.md]

(a) One agent-step of the cfg 4 shard table (Co-GA: pop 50, HoF 10, 2 elites, C = 4, 6 actions: 1010 games) and of the cfg 5
    shard table (Co-ES: pop 250, C = 4, 18 actions: 500 games): two HalfSynthRollouts over one slab, the default route
    (coevo_dqn16_out_synth_step + coevo_dqn16_forward_hidden: three launches) and COEVO_DQN16_FUSED_OUT=0 (coevo_synth_step +
    coevo_dqn16_forward_argmax: four).  Device events around the launches of one round - agent-steps t = 1 and t = 2, one of
    each parity, on a rollout whose t = 0 has run - halved.  After the warm-up the variants alternate untimed until
    --settle-ms have passed, then alternate for --repeats timed rounds each; medians and min .. max.
(c) Whole generations of HalfDQNGAEngine (captured generation replayed) and HalfDQNESEngine on those shapes with T = 200, both
    routes alternating in one process, host clock around the generation + device synchronise: the four-launch engine is the
    parent commit's engine (profiles/r14_fp16_dqn_breeding.md, profiles/r18_fp16_dqn_es.md hold its figures).
(b) Whole generations of DQNGATrainer and DQNESTrainer (collect=False), args.precision float16 against float32, same shapes,
    alternating, host clock around step() + device synchronise.

A per-kernel split comes from a run of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_dqn_train_precision.py --only steps --repeats 5
Run each measurement as one GPU step under its own time limit."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import lib as L   # noqa: E402

DEV = "cuda"
ROLES = ("first_0", "second_0")
SHAPES = {"cfg 4 shard (Co-GA)": dict(kind="ga", pop=50, hof=10, elites=2, C=4, n=6, game="pong_v3"),
          "cfg 5 shard (Co-ES)": dict(kind="es", pop=250, C=4, n=18, game="boxing_v2")}
KNOB = "COEVO_DQN16_FUSED_OUT"


def half_valued_nets(count, C, n_act, seed):
    """[count][P] fp32 flats whose every entry is an fp16 value; BatchNorm weights near 1"""
    P = int(L.load().coevo_dqn_param_count(C, n_act))
    g = torch.Generator(device=DEV).manual_seed(seed)
    flat = torch.randn(count, P, device=DEV, generator=g) * 0.02
    for lo, hi in ((P - 320, P - 288), (P - 256, P - 192), (P - 128, P - 64)):   # vbn*.weight
        flat[:, lo:hi] += 1.0
    return flat.to(torch.float16).to(torch.float32).cpu().numpy()


def with_knob(value, make):
    old = os.environ.pop(KNOB, None)
    if value is not None:
        os.environ[KNOB] = value
    try:
        return make()
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


def half_engine(shape, T, fused):
    """the float16 engine of a shape with its nets loaded and every game live"""
    from coevonet_amd.dqn_es_half import HalfDQNESEngine
    from coevonet_amd.dqn_ga_half import HalfDQNGAEngine
    from coevonet_amd.population import eval_gate_limits
    s = shape
    if s["kind"] == "ga":
        eng = with_knob(None if fused else "0", lambda: HalfDQNGAEngine(s["pop"], s["hof"], s["elites"], s["C"], s["n"], T, T,
                                                                        device=DEV, capacity=4096))
        eng.load_initial({r: half_valued_nets(s["pop"], s["C"], s["n"], 20 + i) for i, r in enumerate(ROLES)},
                         {r: half_valued_nets(s["hof"], s["C"], s["n"], 30 + i) for i, r in enumerate(ROLES)})
        eng.ro.set_limits(eval_gate_limits(eng.ro.n_games, eng.n_main, T, T, 1))
    else:
        eng = with_knob(None if fused else "0", lambda: HalfDQNESEngine(s["pop"], s["C"], s["n"], T, T, device=DEV))
        for i, r in enumerate(ROLES):
            eng.upload(r, "base", 0, half_valued_nets(1, s["C"], s["n"], 40 + i))
        eng.perturb(0, (0.05, 0.05))
    assert eng.ro.fused_out is fused
    torch.cuda.synchronize()
    return eng


def stats(ms):
    ms = np.array(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def verdict(name_a, a, name_b, b):
    """a, b: (median, min, max)"""
    if a[2] < b[1]:
        return f"{name_a} is faster, ranges disjoint"
    if b[2] < a[1]:
        return f"{name_b} is faster, ranges disjoint"
    return "the ranges overlap: equal within the spread"


def alternate(variants, one, a, settle=True):
    """warm-up, settling, then --repeats alternating timed calls of one(variant, timed)"""
    for _ in range(a.warmup):
        for v in variants:
            one(v, False)
    t0, rounds = time.perf_counter(), 0
    while settle and (time.perf_counter() - t0) * 1e3 < a.settle_ms:
        for v in variants:
            one(v, False)
        rounds += 1
    for _ in range(a.repeats):
        for v in variants:   # alternating: a drift of the clocks lands on both alike
            one(v, True)
    return rounds


# ---------------------------------------------------------------------------------------------------- (a) one agent-step
def agent_steps(a):
    lines = ["## (a) One agent-step of the float16 rollout: fused output layer against the four-launch route", ""]
    for title, shape in SHAPES.items():
        variants = []
        for name, fused in (("fused (3 launches)", True), (f"{KNOB}=0 (4 launches)", False)):
            eng = half_engine(shape, a.T, fused)
            ro = eng.ro
            ln, stream = ro.lanes[0], torch.cuda.current_stream().cuda_stream
            ro.enqueue_step(ln, 0, a.T, None, stream)   # reset + the frames of t = 0 (+ their forward)
            variants.append({"name": name, "eng": eng, "ro": ro, "ln": ln, "stream": stream, "ms": []})
        torch.cuda.synchronize()

        def one(v, timed):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            v["ro"].enqueue_step(v["ln"], 1, a.T, None, v["stream"])
            v["ro"].enqueue_step(v["ln"], 2, a.T, None, v["stream"])
            e1.record()
            e1.synchronize()
            if timed:
                v["ms"].append(e0.elapsed_time(e1) * 1e3 / 2)   # us per agent-step
        rounds = alternate(variants, one, a)
        for v in variants:
            L.raise_on_status(v["ro"].status)
        st = [stats(v["ms"]) for v in variants]
        lines += [f"### {title}", "",
                  f"{variants[0]['ro'].n_games} games, C = {shape['C']}, {shape['n']} actions, tasks per parity "
                  f"{variants[0]['ln']['n_tasks']}; warm-up {a.warmup}, {rounds} settling rounds ({a.settle_ms:.0f} ms), {a.repeats} "
                  "alternating timed rounds of each variant (t = 1 and t = 2, halved).", "",
                  "| route | median us / agent-step | min .. max us |", "|---|---|---|"]
        for v, s in zip(variants, st):
            lines.append(f"| {v['name']} | {s[0]:.2f} | {s[1]:.2f} .. {s[2]:.2f} |")
        lines += ["", f"fused / four-launch median: {st[0][0] / st[1][0]:.3f}: " + verdict("the fused route", st[0], "the four-launch route", st[1]), ""]
        for v in variants:
            v["eng"].close()
        del variants
        torch.cuda.empty_cache()
    return lines


# ----------------------------------------------------------------------------------- (c) the engines, both routes
def engines(a):
    lines = ["## (c) Whole float16 engine generations: fused route against the four-launch route (the parent commit's engine)", ""]
    for title, shape in SHAPES.items():
        variants = [{"name": name, "eng": half_engine(shape, a.T, fused), "ms": [], "gen": 0}
                    for name, fused in (("fused (3 launches)", True), (f"{KNOB}=0 (4 launches)", False))]

        def one(v, timed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if shape["kind"] == "ga":
                v["eng"].step(use_graph=True)
            else:
                v["eng"].generation(v["gen"], (0.05, 0.05), 0.1, False)
                v["gen"] += 1
            torch.cuda.synchronize()
            if timed:
                v["ms"].append((time.perf_counter() - t0) * 1e3)
        alternate(variants, one, a, settle=False)
        st = [stats(v["ms"]) for v in variants]
        cls = type(variants[0]["eng"]).__name__
        lines += [f"### {title}: {cls}", "",
                  f"T = {a.T} agent-steps, {variants[0]['eng'].steps_per_generation} agent-steps per generation; warm-up {a.warmup} "
                  f"generations, {a.repeats} alternating timed generations of each route, host clock + device synchronise.", "",
                  "| route | median ms / generation | min .. max ms | generations/s (median) |", "|---|---|---|---|"]
        for v, s in zip(variants, st):
            lines.append(f"| {v['name']} | {s[0]:.2f} | {s[1]:.2f} .. {s[2]:.2f} | {1e3 / s[0]:.2f} |")
        lines += ["", f"fused / four-launch median: {st[0][0] / st[1][0]:.3f}: " + verdict("the fused route", st[0], "the four-launch route", st[1]), ""]
        for v in variants:
            v["eng"].close()
        del variants
        torch.cuda.empty_cache()
    return lines


# --------------------------------------------------------------------------- (b) the trainers, float16 against float32
def trainer_args(shape, precision, a):
    return types.SimpleNamespace(
        game=shape["game"], precision=precision, population=shape["pop"], hof_size=shape.get("hof", 1),
        elites_number=shape.get("elites", 1), max_timesteps_per_episode=a.T, max_evaluation_steps=a.T,
        generations=a.warmup + a.repeats, adaptive=True, mutation_power_agent_0=0.05, mutation_power_agent_1=0.05,
        mutation_power_adversary=0.05, min_mutation_power=0.001, max_mutation_power=0.2, learning_rate=0.1, fitness_sharing=False,
        coevo_channels=shape["C"], render=False)


def trainers(a):
    from coevonet_amd import dqn_population as dp
    from coevonet_amd.game_logic import initialize_env
    lines = ["## (b) Whole trainer generations (collect=False): args.precision float16 against float32", ""]
    for title, shape in SHAPES.items():
        cls = dp.DQNGATrainer if shape["kind"] == "ga" else dp.DQNESTrainer
        variants = []
        for precision in ("float32", "float16"):
            args = trainer_args(shape, precision, a)
            torch.manual_seed(3)
            tr = cls(initialize_env(args), args, collect=False)
            variants.append({"name": f"{precision} ({type(tr.eng).__name__})", "tr": tr, "ms": []})

        def one(v, timed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v["tr"].step()
            torch.cuda.synchronize()
            if timed:
                v["ms"].append((time.perf_counter() - t0) * 1e3)
        alternate(variants, one, a, settle=False)
        for v in variants:
            v["tr"].finish()
        st = [stats(v["ms"]) for v in variants]
        lines += [f"### {title}: {cls.__name__}", "",
                  f"T = {a.T}, {variants[0]['tr'].eng.steps_per_generation} agent-steps per generation; warm-up {a.warmup} "
                  f"generations, {a.repeats} alternating timed generations of each precision, host clock around step() + device "
                  "synchronise.", "", "| precision (engine) | median ms / generation | min .. max ms | generations/s (median) |",
                  "|---|---|---|---|"]
        for v, s in zip(variants, st):
            lines.append(f"| {v['name']} | {s[0]:.2f} | {s[1]:.2f} .. {s[2]:.2f} | {1e3 / s[0]:.2f} |")
        r = np.array(variants[1]["ms"]) / st[0][0]
        lines += ["", f"fp16 / fp32 median generation time: {st[1][0] / st[0][0]:.3f} (fp16 generations over the fp32 median: "
                  f"{r.min():.3f} .. {r.max():.3f}): " + verdict("float16", st[1], "float32", st[0]), ""]
        for v in variants:
            v["tr"].close()
        del variants
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--only", choices=("steps", "engines", "trainers"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats of each variant"
    lines = [f"# float16 DeepQN training: fused env step and trainers ({torch.cuda.get_device_name(0)})", ""]
    for name, section in (("steps", agent_steps), ("engines", engines), ("trainers", trainers)):
        if a.only in (None, name):
            lines += section(a)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
