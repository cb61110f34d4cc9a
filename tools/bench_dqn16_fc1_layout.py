#!/usr/bin/env python3
"""The tiled fc1 block of the fp16 DeepQN slab against the streamed one and against float32 (tiled), from the same nets:

    python tools/bench_dqn16_fc1_layout.py [--repeats 15] [--warmup 3] [--settle-ms 120] [--no-engines] [--only-forward] [--out FILE.md]

Forward: the cfg 4 agent-step table of tools/bench_dqn_shapes.py (1010 rows, 90 tasks, 60 nets, C = 4, 6 actions), every
parameter an fp16 value.  Three variants in one process - fp16 tiled (coevo_dqn16_forward_*_tiled), fp16 streamed
(coevo_dqn16_forward_*), fp32 tiled (coevo_dqn_forward_* with COEVO_DQN_FC1_TILED) - each timed as the whole forward (three
launches) and as the hidden pair (conv stack + fc1, two launches: what a rollout enqueues per agent-step).  The fc1 launch on its
own has no timed entry point in float16: its time is the per-kernel mean of a run of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_dqn16_fc1_layout.py --only-forward --repeats 7
Breeding: 2 roles x 49 children from 2 elites with the stale-agent distances fused in + the finalize, tiled against streamed.
Generations: pop 50, HoF 10, 2 elites, C = 4, T = 200 for HalfDQNGAEngine tiled, HalfDQNGAEngine streamed and DQNGAEngine.

The protocol of tools/bench_dqn_precision.py: after the warm-up the variants alternate (untimed) until --settle-ms of work has
passed, then alternate for --repeats timed rounds each (device events; the generations: host clock around replay + device
synchronise); medians with the min .. max spread.  Run it as one GPU step under its own time limit."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from coevonet_amd import lib as L   # noqa: E402
from bench_dqn_breed_precision import alternate, half_valued_nets   # noqa: E402
from bench_dqn_precision import table   # noqa: E402

DEV = "cuda"
ROWS = L.DQN_MAX_ROWS
ROLES = 2


def spread(label, xs, unit):
    xs = np.array(xs)
    return f"| {label} | {np.median(xs):.{1 if unit == 'us' else 3}f} | {xs.min():.{1 if unit == 'us' else 3}f} .. {xs.max():.{1 if unit == 'us' else 3}f} |"


def compare(name, a, b):
    """`a` against `b` (lists of times): the ratio of the medians and whether the two min .. max ranges are disjoint"""
    a, b = np.array(a), np.array(b)
    r = float(np.median(a) / np.median(b))
    if a.max() < b.min():
        word = "faster, disjoint ranges"
    elif a.min() > b.max():
        word = "slower, disjoint ranges"
    else:
        word = "equal within the spread (overlapping ranges)"
    return f"{name}: ratio of medians {r:.3f} - {word}"


# ----------------------------------------------------------------------------------------------------------------- forward
def forward_variant(name, precision, tiled, flat, layout, C, n_act, frames, hidden):
    lib = L.load()
    half = precision == "float16"
    sym = "coevo_dqn16" if half else "coevo_dqn"
    Cw = C if half else C | (L.DQN_FC1_TILED if tiled else 0)
    n_nets = flat.shape[0]
    stride = int(getattr(lib, sym + "_slab_stride")(C, n_act))
    slab = torch.zeros(n_nets, stride, dtype=torch.int32 if half else torch.float32, device=DEV)
    L.call(sym + "_pack" + ("_tiled" if half and tiled else ""), L._p(flat), L._p(slab), n_nets, Cw, n_act)
    tasks = np.zeros(len(layout), dtype=L.DQN_TASK_DTYPE)
    row = 0
    for i, (net, r) in enumerate(layout):
        tasks[i] = (net * stride, row, r)
        row += r
    d_tasks = L.tasks_to_device(tasks, DEV)
    actions = torch.zeros(row, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(int(getattr(lib, sym + "_workspace_bytes")(row)) // 4, dtype=torch.float32, device=DEV)
    sfx = "_tiled" if half and tiled else ""
    stream = torch.cuda.current_stream().cuda_stream
    head = (L._p(slab), L._p(d_tasks), len(layout), ROWS, row, Cw, n_act, L._p(frames))
    if hidden and half:
        fn, tail = getattr(lib, sym + "_forward_hidden" + sfx), (L._p(status), L._p(ws), stream)
    elif hidden:
        fn, tail = lib.coevo_dqn_forward_hidden_timed, (L._p(ws), None, 0, stream)   # (no timing context: the plain pair)
    else:
        fn, tail = getattr(lib, sym + "_forward_argmax" + sfx), (L._p(actions), None, L._p(status), L._p(ws), stream)
    return {"name": name + (" hidden pair" if hidden else " whole forward"), "run": lambda: L._check(fn(*head, *tail), name),
            "ms": [], "keep": (slab, d_tasks, actions, status, ws), "status": status, "actions": actions,
            "mb": 4 * stride * n_nets / 1e6}


def forward(a):
    n_act, n_nets, layout = table("cfg4")
    flat = half_valued_nets(n_nets, a.C, n_act, 7)
    rows = sum(r for _, r in layout)
    g = torch.Generator(device=DEV).manual_seed(9)
    frames = torch.randint(0, 256, (rows, 84, 84, a.C), dtype=torch.uint8, device=DEV, generator=g)
    kinds = (("fp16 tiled", "float16", True), ("fp16 streamed", "float16", False), ("fp32 tiled", "float32", True))
    variants = [forward_variant(nm, p, t, flat, layout, a.C, n_act, frames, hidden) for hidden in (False, True) for nm, p, t in kinds]
    del flat
    settle = alternate(variants, a)
    for v in variants:
        assert int(v["status"].item()) == 0, v["name"]
    assert torch.equal(variants[0]["actions"], variants[1]["actions"]), "fp16 tiled and fp16 streamed act differently"
    lines = [f"## Forward on the cfg 4 agent-step table: {rows} rows, {len(layout)} tasks, {n_nets} nets, C = {a.C}, {n_act} actions", "",
             f"warm-up {a.warmup}, {settle} settling rounds ({a.settle_ms:.0f} ms), {a.repeats} alternating timed repeats of each "
             "variant, device events; the actions of fp16 tiled and fp16 streamed are equal on every row.", "",
             "| variant | median us | min .. max us |", "|---|---|---|"]
    us = {v["name"]: [m * 1e3 for m in v["ms"]] for v in variants}
    lines += [spread(f"{v['name']} ({v['mb']:.0f} MB of weights)", us[v["name"]], "us") for v in variants]
    lines += [""] + [compare(f"{x} against {y}", us[x], us[y]) for x, y in
                     (("fp16 tiled whole forward", "fp16 streamed whole forward"), ("fp16 tiled whole forward", "fp32 tiled whole forward"),
                      ("fp16 tiled hidden pair", "fp16 streamed hidden pair"), ("fp16 tiled hidden pair", "fp32 tiled hidden pair"))] + [""]
    return lines


# ---------------------------------------------------------------------------------------------------------------- breeding
def breeding_variant(tiled, flats, pop, E, C, n_act):
    lib = L.load()
    stride, nb = int(lib.coevo_dqn16_slab_stride(C, n_act)), int(lib.coevo_dqn16_perturb_blocks(C, n_act))
    idx = torch.tensor([c % E for c in range(pop - 1)], dtype=torch.int32, device=DEV)
    sfx = "_tiled" if tiled else ""
    keep = []
    for ri in range(ROLES):   # per role [elite E | stale 1 | pop]
        slab = torch.zeros((E + 1 + pop) * stride, dtype=torch.int32, device=DEV)
        L.call("coevo_dqn16_pack" + sfx, L._p(flats[ri]), L._p(slab), E + 1, C, n_act)
        keep.append({"slab": slab, "part": torch.zeros((pop - 1) * nb, dtype=torch.float64, device=DEV),
                     "dist": torch.zeros(pop, dtype=torch.float32, device=DEV), "head": torch.zeros(1, dtype=torch.float32, device=DEV),
                     "sigma": torch.full((1,), 0.05, dtype=torch.float32, device=DEV)})
    at = lambda k, net: k["slab"].data_ptr() + 4 * net * stride   # noqa: E731

    def run():
        for ri, k in enumerate(keep):
            L.call("coevo_dqn16_perturb_dist" + sfx, at(k, 0), L._p(idx), at(k, E + 1), 1, pop - 1, C, n_act, L._p(k["sigma"]), 0, 0,
                   ri, 0, None, 0, at(k, E), L._p(k["part"]))
            L.call("coevo_fc16_distance_finalize", L._p(k["part"]), nb, pop - 1, L._p(k["dist"]), 1, L._p(k["head"]))
    return {"name": "fp16 tiled" if tiled else "fp16 streamed", "run": run, "ms": [], "keep": (keep, idx),
            "dist": [k["dist"] for k in keep], "bytes": ROLES * 4 * stride * (pop - 1)}


def breeding(a):
    flats = [half_valued_nets(a.elites + 1, a.C, a.actions, 8 + ri) for ri in range(ROLES)]
    variants = [breeding_variant(t, flats, a.pop, a.elites, a.C, a.actions) for t in (True, False)]
    settle = alternate(variants, a)
    same = all(torch.equal(x, y) for x, y in zip(variants[0]["dist"], variants[1]["dist"]))
    lines = ["## Breeding launches of one generation", "",
             f"{ROLES} roles x {a.pop - 1} children from {a.elites} elites, stale-agent distances fused in, + coevo_fc16_distance_finalize; "
             f"{variants[0]['bytes'] / 1e6:.0f} MB of children written; warm-up {a.warmup}, {settle} settling rounds, {a.repeats} "
             f"alternating timed repeats; the finalized distances of the two layouts are {'equal' if same else 'NOT equal'}.", "",
             "| variant | median ms | min .. max ms |", "|---|---|---|"]
    lines += [spread(v["name"], v["ms"], "ms") for v in variants]
    lines += ["", compare("fp16 tiled against fp16 streamed", variants[0]["ms"], variants[1]["ms"]), ""]
    return lines


# ------------------------------------------------------------------------------------------------------------- generations
def generations(a):
    from coevonet_amd.dqn_ga_half import HalfDQNGAEngine
    from coevonet_amd.dqn_population import DQNGAEngine
    roles = ("first_0", "second_0")
    pop_flat = {r: half_valued_nets(a.pop, a.C, a.actions, 20 + i).cpu().numpy() for i, r in enumerate(roles)}
    hof_flat = {r: half_valued_nets(a.hof, a.C, a.actions, 30 + i).cpu().numpy() for i, r in enumerate(roles)}
    shape = (a.pop, a.hof, a.elites, a.C, a.actions, a.T, a.T)
    engines = []
    for name, make in (("HalfDQNGAEngine tiled", lambda: HalfDQNGAEngine(*shape, device=DEV, capacity=4096, fc1_layout="tiled")),
                       ("HalfDQNGAEngine streamed", lambda: HalfDQNGAEngine(*shape, device=DEV, capacity=4096)),
                       ("DQNGAEngine (float32, tiled fc1)", lambda: DQNGAEngine(*shape, device=DEV, capacity=4096))):
        eng = make()
        eng.load_initial(pop_flat, hof_flat)
        engines.append({"name": name, "eng": eng, "ms": []})

    def step(e, timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e["eng"].step(use_graph=True)
        torch.cuda.synchronize()
        if timed:
            e["ms"].append((time.perf_counter() - t0) * 1e3)
    for _ in range(a.warmup):
        for e in engines:
            step(e, False)
    for _ in range(a.gen_repeats):
        for e in engines:
            step(e, True)
    for e in engines:
        L.raise_on_status(e["eng"].ro.status)
    t, s = engines[0]["eng"], engines[1]["eng"]
    same = torch.equal(t.ro.acc, s.ro.acc) and all(torch.equal(x, y) for x, y in zip(t.fitness, s.fitness))
    lines = ["## Whole generations", "",
             f"pop {a.pop}, HoF {a.hof}, {a.elites} elites, C = {a.C}, {a.actions} actions, T = {a.T} "
             f"({t.steps_per_generation} agent-steps per generation), the captured generation replayed; warm-up {a.warmup} generations, "
             f"{a.gen_repeats} alternating timed generations of each engine, host clock around replay + device synchronise; rewards "
             f"and fitness of the two float16 engines after the last generation are {'equal' if same else 'NOT equal'}.", "",
             "| engine | median ms / generation | min .. max ms |", "|---|---|---|"]
    lines += [spread(e["name"], e["ms"], "ms") for e in engines]
    lines += ["", compare("HalfDQNGAEngine tiled against HalfDQNGAEngine streamed", engines[0]["ms"], engines[1]["ms"]),
              compare("HalfDQNGAEngine tiled against DQNGAEngine", engines[0]["ms"], engines[2]["ms"]),
              compare("HalfDQNGAEngine streamed against DQNGAEngine", engines[1]["ms"], engines[2]["ms"]), ""]
    for e in engines:
        e["eng"].ro.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=50)
    ap.add_argument("--hof", type=int, default=10)
    ap.add_argument("--elites", type=int, default=2)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--actions", type=int, default=6)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--gen-repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--only-forward", action="store_true", help="the forward variants only (the form to run under rocprofv3)")
    ap.add_argument("--no-engines", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 7 and a.gen_repeats >= 5, "at least 7 repeats of each launch variant and 5 of each engine"
    lines = [f"# fc1 layout of the fp16 DeepQN slab: tiled against streamed and float32 ({torch.cuda.get_device_name(0)})", ""]
    lines += forward(a)
    torch.cuda.empty_cache()
    if not a.only_forward:
        lines += breeding(a)
        torch.cuda.empty_cache()
        if not a.no_engines:
            lines += generations(a)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
